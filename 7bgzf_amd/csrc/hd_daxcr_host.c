/*
 * hd_daxcr_host.c -- hd7daxcr: applet/7daxcr.c (_compress :72-176, _decompress
 * :178-239) over libhipdeflate.so.  DAX: a 32-byte header, a table of 32-bit file
 * offsets and one of 16-bit sizes, then every 8192-byte frame as its own RFC 1950
 * (zlib) stream -- the container that goes through zlibutil_buffer_code's rfc1950
 * wrapper (lib/zlibutil.c:374-397) in the reference.
 *
 *     hd7daxcr -G<level> dec.iso enc.dax
 *     hd7daxcr -d < enc.dax > dec.iso
 *
 * What changed, and why: frames go to the device 32,768 at a time and come back as
 * finished zlib members (HD_FRAME_ZLIB: 78 da, the stream, Adler-32 computed on the
 * device).  The reader inflates the members' payloads in batches; non-compressed
 * areas (which neither writer makes) are honoured.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "hd_host_batch.h"

#define DX_BLOCK 8192u
#define DX_BATCH 32768u

static int dx_compress(FILE *in, FILE *out, int level)
{
	const long long total = file_size(in);
	if (total < 0 || total >= (1ll << 32)) {
		fprintf(stderr, total < 0 ? "cannot stat the input\n" : "input too large for a DAX header\n");
		return 2;
	}
	const uint32_t nblk = (uint32_t)((total + DX_BLOCK - 1) / DX_BLOCK);
	unsigned char hdr[32] = { 'D', 'A', 'X', 0 };
	wr32(hdr + 4, (uint32_t)total);
	wr32(hdr + 8, 1);
	struct hd_batch b;
	int ret = hd_batch_open(&b, DX_BATCH, (size_t)DX_BATCH * DX_BLOCK, hipdeflate_bound(DX_BLOCK, level), 0);
	unsigned char *index = calloc(6, (size_t)nblk + 1);
	if (!ret && !index) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
	}
	if (ret)
		goto out;
	unsigned char *sizes = index + 4 * (size_t)nblk;
	fwrite(hdr, 1, 32, out);
	fwrite(index, 1, 6 * (size_t)nblk, out);
	uint64_t pos = 32 + 6 * (uint64_t)nblk;
	long long left = total;
	for (uint32_t c = 0; c < nblk; c += DX_BATCH) {
		const uint32_t n = nblk - c < DX_BATCH ? nblk - c : DX_BATCH;
		if ((ret = hd_batch_read(&b, in, n, DX_BLOCK, &left)) || (ret = hd_batch_deflate(&b, n, level, HD_FRAME_ZLIB, HD_FRAME_ZLIB)))
			goto out;
		for (uint32_t i = 0; i < n; i++) {
			if (b.olen[i] > 0xffff) {
				fprintf(stderr, "hip_deflate 1\n");
				ret = 1;
				goto out;
			}
			if (pos >= (1ull << 32)) {
				fprintf(stderr, "output too large for 32-bit DAX offsets\n");
				ret = 2;
				goto out;
			}
			wr32(index + 4 * (size_t)(c + i), (uint32_t)pos);
			wr16(sizes + 2 * (size_t)(c + i), b.olen[i]);
			fwrite(b.out + (size_t)i * b.stride, 1, b.olen[i], out);
			pos += b.olen[i];
		}
		fprintf(stderr, "%u / %u\r", c + n, nblk);
	}
	fseeko(out, 32, SEEK_SET);
	fwrite(index, 1, 6 * (size_t)nblk, out);
	fprintf(stderr, "%u / %u done.\n", nblk, nblk);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(index);
	return ret;
}

static int dx_decompress(FILE *in, FILE *out)
{
	unsigned char hdr[32];
	if (read_full(in, hdr, 32) != 32 || memcmp(hdr, "DAX\0", 4)) {
		fprintf(stderr, "not DAX\n");
		return 1;
	}
	const uint32_t total = rd32(hdr + 4), nnc = rd32(hdr + 12);
	const uint32_t nblk = (uint32_t)(((uint64_t)total + DX_BLOCK - 1) / DX_BLOCK);
	if (nnc > nblk) {
		fprintf(stderr, "not DAX\n");
		return 1;
	}
	struct hd_batch b;
	int ret = hd_batch_open(&b, DX_BATCH, (size_t)DX_BATCH * (DX_BLOCK + 64), DX_BLOCK, 0);
	unsigned char *index = malloc(6 * (size_t)nblk + 8 * (size_t)nnc + 16);
	/* frames of the non-compressed areas: plain 8192-byte frames in the file (:194-203) */
	unsigned char *plain = calloc(1, (size_t)nblk + 1);
	if (ret)
		goto out;
	if (!index || read_full(in, index, 6 * (size_t)nblk + 8 * (size_t)nnc) != 6 * (size_t)nblk + 8 * (size_t)nnc) {
		fprintf(stderr, "unexpected end of file\n");
		ret = 1;
		goto out;
	}
	if (!plain) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
		goto out;
	}
	const unsigned char *sizes = index + 4 * (size_t)nblk, *nc = sizes + 2 * (size_t)nblk;
	for (uint32_t k = 0; k < nnc; k++) {
		const uint32_t first = rd32(nc + 8 * (size_t)k), cnt = rd32(nc + 8 * (size_t)k + 4);
		for (uint32_t j = 0; j < cnt && (uint64_t)first + j < nblk; j++)
			plain[first + j] = 1;
	}
	uint64_t produced = 0;
	for (uint32_t c = 0; c < nblk; c += DX_BATCH) {
		const uint32_t m = nblk - c < DX_BATCH ? nblk - c : DX_BATCH;
		size_t itotal = 0;
		uint32_t nz = 0;
		for (uint32_t i = 0; i < m; i++) {
			const uint32_t want = (uint64_t)(c + i + 1) * DX_BLOCK <= total ? DX_BLOCK : (uint32_t)(total - (uint64_t)(c + i) * DX_BLOCK);
			const uint32_t sz = plain[c + i] ? DX_BLOCK : rd16(sizes + 2 * (size_t)(c + i));
			if (sz > DX_BLOCK + 64 || (!plain[c + i] && sz < 6)) {
				fprintf(stderr, "corrupted size table\n");
				ret = 1;
				goto out;
			}
			if (!plain[c + i]) {
				b.off[nz] = itotal + 2;                /* behind the two zlib header bytes */
				b.len[nz] = sz - 2;                    /* the Adler-32 rides along as trailing bytes */
				b.ooff[nz] = (uint64_t)i * DX_BLOCK;
				b.cap[nz++] = want;
			}
			itotal += sz;
		}
		if (read_full(in, b.in, itotal) != itotal) {
			fprintf(stderr, "unexpected end of file\n");
			ret = 1;
			goto out;
		}
		size_t at = 0;
		for (uint32_t i = 0; i < m; i++) {
			if (plain[c + i]) {
				memcpy(b.out + (size_t)i * DX_BLOCK, b.in + at, DX_BLOCK);
				at += DX_BLOCK;
			} else {
				if ((b.in[at] & 0x0f) != 8 || ((b.in[at] << 8) | b.in[at + 1]) % 31) {
					fprintf(stderr, "frame %u is not a zlib stream\n", c + i);
					ret = 1;
					goto out;
				}
				at += rd16(sizes + 2 * (size_t)(c + i));
			}
		}
		if ((ret = hd_batch_inflate(&b, nz, 0)))
			goto out;
		for (uint32_t k = 0; k < nz; k++) {
			if (b.olen[k] != b.cap[k]) {
				fprintf(stderr, "inflate 1\n");
				ret = 1;
				goto out;
			}
		}
		const uint64_t bytes = produced + (uint64_t)m * DX_BLOCK <= total ? (uint64_t)m * DX_BLOCK : total - produced;
		fwrite(b.out, 1, (size_t)bytes, out);
		produced += bytes;
		fprintf(stderr, "%u / %u\r", c + m, nblk);
	}
	fprintf(stderr, "%u / %u done.\n", nblk, nblk);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(index);
	free(plain);
	return ret;
}

int main(int argc, char **argv)
{
	struct hd_host_args a;
	hd_host_parse(&a, argc, argv, NULL);
	if (a.bad || (a.decode && (a.n || a.level >= 0)) || (!a.decode && (a.n != 2 || a.level < 0 || a.level > 9)) ||
	    (a.decode && (isatty(0) || isatty(1)))) {
		fprintf(stderr, "usage: %s -G<level> dec.iso enc.dax   or   -d < enc.dax > dec.iso\n", argv[0]);
		return 1;
	}
	double t0;
	int ret = hd_host_begin(&t0);
	if (ret)
		return ret;
	if (a.decode) {
		ret = dx_decompress(stdin, stdout);
	} else {
		FILE *in = fopen(a.name[0], "rb");
		if (!in) {
			fprintf(stderr, "failed to open %s\n", a.name[0]);
			return 2;
		}
		FILE *out = fopen(a.name[1], "wb");
		if (!out) {
			fprintf(stderr, "failed to open %s\n", a.name[1]);
			fclose(in);
			return 3;
		}
		fprintf(stderr, "compression level = %d (hip)\n", a.level);
		ret = dx_compress(in, out, a.level);
		fclose(in);
		if (fclose(out) && !ret)
			ret = 2;
	}
	return hd_host_end(t0, ret);
}
