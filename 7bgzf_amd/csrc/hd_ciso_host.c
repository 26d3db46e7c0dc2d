/*
 * hd_ciso_host.c -- hd7ciso: applet/7ciso.c (_compress :81-208, _decompress
 * :210-293) over libhipdeflate.so.  CISO: a 24-byte header, a table of
 * (sectors + 1) 32-bit file offsets (bit 31 = the sector is stored as it is), then
 * every 2048-byte sector as its own raw DEFLATE stream.  The tiny-block end of the
 * path: a 1 GiB image is 524,288 independent blocks.
 *
 *     hd7ciso -G<level> [-t<percent>] dec.iso enc.cso
 *     hd7ciso -d < enc.cso > dec.iso
 *
 * What changed, and why: sectors go to the device 65,536 at a time in one call
 * (the reference: one pthread per sector); a sector whose stream is longer than
 * threshold % of 2048 is written plain, as there (:188-193).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "hd_host_batch.h"

#define CS_BLOCK 2048u
#define CS_BATCH 65536u

static int cs_compress(FILE *in, FILE *out, int level, int threshold)
{
	const long long total = file_size(in);
	if (total < 0 || total >= (1ll << 31)) {
		fprintf(stderr, total < 0 ? "cannot stat the input\n" : "input too large for 31-bit CISO offsets\n");
		return 2;
	}
	const uint32_t nblk = (uint32_t)((total + CS_BLOCK - 1) / CS_BLOCK);
	unsigned char hdr[24] = { 'C', 'I', 'S', 'O' };
	wr32(hdr + 4, 24);
	wr32(hdr + 8, (uint32_t)total);
	wr32(hdr + 12, (uint32_t)((uint64_t)total >> 32));
	wr32(hdr + 16, CS_BLOCK);
	hdr[20] = 1;                                     /* ver; align = 0 */
	struct hd_batch b;
	int ret = hd_batch_open(&b, CS_BATCH, (size_t)CS_BATCH * CS_BLOCK, up16(CS_BLOCK + 5 + 32), 0);
	unsigned char *index = calloc(4, (size_t)nblk + 1);
	if (!ret && !index) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
	}
	if (ret)
		goto out;
	fwrite(hdr, 1, 24, out);
	fwrite(index, 4, (size_t)nblk + 1, out);
	uint64_t pos = 24 + 4 * ((uint64_t)nblk + 1);
	long long left = total;
	for (uint32_t c = 0; c < nblk; c += CS_BATCH) {
		const uint32_t n = nblk - c < CS_BATCH ? nblk - c : CS_BATCH;
		if ((ret = hd_batch_read(&b, in, n, CS_BLOCK, &left)) || (ret = hd_batch_deflate(&b, n, level, HD_FRAME_RAW, HD_FRAME_RAW)))
			goto out;
		for (uint32_t i = 0; i < n; i++) {
			if (pos >= (1ull << 31)) {
				fprintf(stderr, "output too large for 31-bit CISO offsets\n");
				ret = 2;
				goto out;
			}
			if (b.olen[i] > CS_BLOCK * (uint32_t)threshold / 100) {
				wr32(index + 4 * (size_t)(c + i), 0x80000000u | (uint32_t)pos);
				fwrite(b.in + b.off[i], 1, b.len[i], out);
				pos += b.len[i];
			} else {
				wr32(index + 4 * (size_t)(c + i), (uint32_t)pos);
				fwrite(b.out + (size_t)i * b.stride, 1, b.olen[i], out);
				pos += b.olen[i];
			}
		}
		fprintf(stderr, "%u / %u\r", c + n, nblk);
	}
	wr32(index + 4 * (size_t)nblk, (uint32_t)pos);
	fseeko(out, 24, SEEK_SET);
	fwrite(index, 4, (size_t)nblk + 1, out);
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

static int cs_decompress(FILE *in, FILE *out)
{
	unsigned char hdr[24];
	if (read_full(in, hdr, 24) != 24 || memcmp(hdr, "CISO", 4) || (rd32(hdr + 4) && rd32(hdr + 4) != 24)) {
		fprintf(stderr, "not CISO\n");
		return 1;
	}
	const uint64_t total = rd32(hdr + 8) | ((uint64_t)rd32(hdr + 12) << 32);
	const uint32_t block = rd32(hdr + 16), align = hdr[21];
	if (!block || block > (1u << 20) || align > 8 || total / block >= (1u << 27)) {
		fprintf(stderr, "not CISO\n");
		return 1;
	}
	const uint32_t nblk = (uint32_t)((total + block - 1) / block);
	/* the sector size comes from the file: a batch holds at most 128 MiB of output whatever it claims (2048-byte
	 * sectors: the whole CS_BATCH; a header that says 1 MiB: 128 of them -- not a 64 GiB allocation) */
	const uint32_t batch = (uint32_t)((128u << 20) / up16(block)) < CS_BATCH ? (uint32_t)((128u << 20) / up16(block)) : CS_BATCH;
	struct hd_batch b;
	int ret = hd_batch_open(&b, batch, 0, up16(block), 0);
	unsigned char *index = malloc(4 * ((size_t)nblk + 1));
	if (ret)
		goto out;
	if (!index || read_full(in, index, 4 * ((size_t)nblk + 1)) != 4 * ((size_t)nblk + 1)) {
		fprintf(stderr, "unexpected end of file\n");
		ret = 1;
		goto out;
	}
	uint64_t at = 24 + 4 * ((uint64_t)nblk + 1);       /* stdin is a pipe: the position is counted, not sought (:216) */
	uint64_t produced = 0;
#define CS_POS(k) ((uint64_t)(rd32(index + 4 * (size_t)(k)) & 0x7fffffffu) << align)
	/* bytes sector i of the batch holds: block, but the last one of the image may be short */
#define CS_WANT(i) (produced + (uint64_t)((i) + 1) * block <= total ? block : (uint32_t)(total - produced - (uint64_t)(i) * block))
	for (uint32_t c = 0; c < nblk; c += batch) {
		const uint32_t m = nblk - c < batch ? nblk - c : batch;
		const uint64_t first = CS_POS(c), end = CS_POS(c + m);
		if (first < at || end < first || end - first > (uint64_t)m * (block + 64)) {
			fprintf(stderr, "corrupted index\n");
			ret = 1;
			goto out;
		}
		const size_t span = (size_t)(end - at);             /* bytes between sectors are skipped, as there (:232) */
		if ((ret = hd_grow(&b.in, &b.icap, span)))
			goto out;
		if (read_full(in, b.in, span) != span) {
			fprintf(stderr, "unexpected end of file\n");
			ret = 1;
			goto out;
		}
		uint32_t nz = 0;
		for (uint32_t i = 0; i < m && !ret; i++) {
			const uint64_t lo = CS_POS(c + i), hi = CS_POS(c + i + 1);
			if (lo < at || hi < lo || hi > end) {
				ret = 1;
			} else if (rd32(index + 4 * (size_t)(c + i)) & 0x80000000u) {
				if (hi - lo < CS_WANT(i))
					ret = 1;
				else
					memcpy(b.out + (size_t)i * b.stride, b.in + (size_t)(lo - at), CS_WANT(i));
			} else {
				b.off[nz] = lo - at;
				b.len[nz] = (uint32_t)(hi - lo);
				b.ooff[nz] = (uint64_t)i * b.stride;
				b.cap[nz++] = block;
			}
		}
		if (ret) {
			fprintf(stderr, "corrupted index\n");
			goto out;
		}
		if ((ret = hd_batch_inflate(&b, nz, 0)))
			goto out;
		for (uint32_t k = 0; k < nz; k++) {
			if (b.olen[k] != CS_WANT(b.ooff[k] / b.stride)) {
				fprintf(stderr, "inflate 1\n");
				ret = 1;
				goto out;
			}
		}
		const uint64_t bytes = produced + (uint64_t)m * block <= total ? (uint64_t)m * block : total - produced;
		if (b.stride == block) {
			fwrite(b.out, 1, (size_t)bytes, out);
		} else {
			for (uint32_t i = 0; i < m; i++) {
				const uint64_t o = (uint64_t)i * block;
				if (o < bytes)
					fwrite(b.out + (size_t)i * b.stride, 1, bytes - o < block ? (size_t)(bytes - o) : block, out);
			}
		}
		produced += bytes;
		at = end;
		fprintf(stderr, "%u / %u\r", c + m, nblk);
	}
#undef CS_WANT
#undef CS_POS
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

int main(int argc, char **argv)
{
	struct hd_host_args a;
	hd_host_parse(&a, argc, argv, "t:");
	if (a.bad || (a.decode && (a.n || a.level >= 0)) || (!a.decode && (a.n != 2 || a.level < 0 || a.level > 9)) ||
	    (a.decode && (isatty(0) || isatty(1)))) {
		fprintf(stderr, "usage: %s -G<level> [-t<percent>] dec.iso enc.cso   or   -d < enc.cso > dec.iso\n", argv[0]);
		return 1;
	}
	int threshold = a.opt ? atoi(a.opt) : 100;
	if (threshold < 10)
		threshold = 10;
	if (threshold > 100)
		threshold = 100;
	double t0;
	int ret = hd_host_begin(&t0);
	if (ret)
		return ret;
	if (a.decode) {
		ret = cs_decompress(stdin, stdout);
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
		ret = cs_compress(in, out, a.level, threshold);
		fclose(in);
		if (fclose(out) && !ret)
			ret = 2;
	}
	return hd_host_end(t0, ret);
}
