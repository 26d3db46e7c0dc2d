/*
 * hd_dictzip_host.c -- hd7dictzip: applet/7dictzip.c (_compress :179-325,
 * _decompress :327-402) over libhipdeflate.so.  Same command line shape and the
 * same file format ("improved dictzip": one gzip member per <= 32762 chunks, an
 * 'RA' extra field holding the compressed size of every chunk, chunks in
 * full-flush form, then an empty final block `03 00`, CRC-32 and ISIZE):
 *
 *     hd7dictzip -G<level> [-X] dec.bin enc.dz       (-X: 0xff00-byte chunks, else 58315)
 *     hd7dictzip -d enc.dz > dec.bin
 *
 * What changed, and why: the reference compresses one chunk per pthread with a
 * final block and then re-inflates it on the CPU with a patched zlib to turn it
 * into full-flush form (zlibutil_buffer_full_flush, :93-126).  Here a batch of
 * chunks goes to the device in one call and the kernel emits the full-flush form
 * itself (HD_FRAME_RAW_FLUSH); the CRC-32 of the whole member is folded from the
 * per-chunk CRCs the kernel returns (the reference runs fcrc32 over the input on
 * the host, :203), and the reader checks it, which the reference's does not.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hd_host_batch.h"

#define DZ_BATCH 2048                 /* chunks per device call */
#define DZ_MAX_CHUNKS 32762           /* (0xffff - 10) / 2, applet/7dictzip.c:180 */

/* ---- compress ---------------------------------------------------------------------- */

static int dz_compress(FILE *in, FILE *out, int level, uint32_t block_size)
{
	const long long max_member = (long long)block_size * DZ_MAX_CHUNKS;
	const long long total = file_size(in);
	if (total < 0) {
		fprintf(stderr, "cannot stat the input\n");
		return 2;
	}
	/* a slot under 65535 bytes: every chunk's size fits the 16-bit table */
	struct hd_batch b;
	int ret = hd_batch_open(&b, DZ_BATCH, (size_t)DZ_BATCH * block_size, up16((size_t)block_size + 5 * (block_size / 65535 + 1) + 32), 1);
	unsigned char *sizes = malloc(2 * DZ_MAX_CHUNKS + 16);
	if (!ret && !sizes) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
	}
	if (ret)
		goto out;
	long long done = 0;
	do {
		const long long cur = total - done < max_member ? total - done : max_member;
		const uint32_t nchunks = (uint32_t)((cur + block_size - 1) / block_size);
		unsigned char hdr[22] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0x03 };
		wr16(hdr + 10, 10 + 2 * nchunks);
		hdr[12] = 'R', hdr[13] = 'A';
		wr16(hdr + 14, 6 + 2 * nchunks);
		wr16(hdr + 16, 1);
		wr16(hdr + 18, block_size);
		wr16(hdr + 20, nchunks);
		fwrite(hdr, 1, 22, out);
		const long long pos_sizes = ftello(out);
		memset(sizes, 0, 2 * (size_t)nchunks);
		fwrite(sizes, 1, 2 * (size_t)nchunks, out);

		struct crc_fold fold = { 0, 0, 0 };
		long long left = cur;
		for (uint32_t c = 0; c < nchunks; c += DZ_BATCH) {
			const uint32_t n = nchunks - c < DZ_BATCH ? nchunks - c : DZ_BATCH;
			if ((ret = hd_batch_read(&b, in, n, block_size, &left)) ||
			    (ret = hd_batch_deflate(&b, n, level, HD_FRAME_RAW_FLUSH, HD_FRAME_RAW_FLUSH)))
				goto out;
			for (uint32_t i = 0; i < n; i++) {
				wr16(sizes + 2 * (size_t)(c + i), b.olen[i]);
				fwrite(b.out + (size_t)i * b.stride, 1, b.olen[i], out);
				crc_append(&fold, b.crc[i], b.len[i]);
			}
			fprintf(stderr, "%u / %u\r", c + n, nchunks);
		}
		const long long pos = ftello(out);
		fseeko(out, pos_sizes, SEEK_SET);
		fwrite(sizes, 1, 2 * (size_t)nchunks, out);
		fseeko(out, pos, SEEK_SET);
		unsigned char trl[10] = { 0x03, 0x00 };     /* empty final block: a plain gzip reader sees a whole member */
		wr32(trl + 2, fold.crc);
		wr32(trl + 6, (uint32_t)cur);
		fwrite(trl, 1, 10, out);
		fprintf(stderr, "%u / %u done.\n", nchunks, nchunks);
		done += cur;
	} while (done < total);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(sizes);
	return ret;
}

/* ---- decompress -------------------------------------------------------------------- */

/* applet/7dictzip.c:137-177: the gzip header with the 'RA' field; returns the header
 * length, 0 if this is not such a header */
static size_t dz_header(const unsigned char *d, size_t size, size_t *sizes_off, uint32_t *block_size, uint32_t *nchunks)
{
	if (size < 12 || d[0] != 0x1f || d[1] != 0x8b || d[2] != 8 || (d[3] & 0xe0) || !(d[3] & 4))
		return 0;
	const uint32_t flags = d[3];
	size_t n = 10;
	const uint32_t xlen = rd16(d + n);
	n += 2;
	if (size < n + xlen || xlen < 10)
		return 0;
	if (!(d[n] == 'R' && d[n + 1] == 'A' && rd16(d + n + 2) + 4 == xlen && d[n + 4] == 1 && d[n + 5] == 0 &&
	      rd16(d + n + 8) * 2 + 10 == xlen))
		return 0;
	*block_size = rd16(d + n + 6);
	*nchunks = rd16(d + n + 8);
	*sizes_off = n + 10;
	n += xlen;
	if (flags & 8)
		while (n < size && d[n++])
			;
	if (flags & 16)
		while (n < size && d[n++])
			;
	if (flags & 2)
		n += 2;
	return n <= size ? n : 0;
}

static int dz_decompress(FILE *in, FILE *out)
{
	const long long fsize = file_size(in);
	struct hd_batch b;
	int ret = hd_batch_open(&b, DZ_BATCH, 0, 0, 1);
	unsigned char *head = malloc(65536 + 280);
	if (!ret && !head) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
	}
	if (ret)
		goto out;
	for (;;) {
		const long long pos = ftello(in);
		if (pos >= fsize)
			break;
		const size_t got = fread(head, 1, 65536 + 280, in);
		size_t sizes_off = 0;
		uint32_t block_size = 0, nchunks = 0;
		const size_t n = dz_header(head, got, &sizes_off, &block_size, &nchunks);
		if (!n || !block_size) {
			fprintf(stderr, "header is not gzip (possibly corrupted)\n");
			ret = 1;
			goto out;
		}
		const unsigned char *sizes = head + sizes_off;
		fseeko(in, pos + (long long)n, SEEK_SET);
		struct crc_fold fold = { 0, 0, 0 };
		uint64_t produced = 0;
		for (uint32_t c = 0; c < nchunks; c += DZ_BATCH) {
			const uint32_t m = nchunks - c < DZ_BATCH ? nchunks - c : DZ_BATCH;
			size_t itotal = 0;
			for (uint32_t i = 0; i < m; i++) {
				b.off[i] = itotal;
				b.len[i] = rd16(sizes + 2 * (size_t)(c + i));
				itotal += b.len[i];
				b.ooff[i] = (uint64_t)i * up16(block_size);
				b.cap[i] = block_size;
			}
			if ((ret = hd_grow(&b.in, &b.icap, itotal)) || (ret = hd_grow(&b.out, &b.ocap, (size_t)m * up16(block_size))))
				goto out;
			if (fread(b.in, 1, itotal, in) != itotal) {
				fprintf(stderr, "unexpected end of file\n");
				ret = 1;
				goto out;
			}
			if ((ret = hd_batch_inflate(&b, m, 1)))
				goto out;
			for (uint32_t i = 0; i < m; i++) {
				fwrite(b.out + b.ooff[i], 1, b.olen[i], out);
				crc_append(&fold, b.crc[i], b.olen[i]);
				produced += b.olen[i];
			}
			fprintf(stderr, "%u / %u\r", c + m, nchunks);
		}
		fprintf(stderr, "%u / %u done.\n", nchunks, nchunks);
		/* trailer: `03 00` (ours and the reference's writer) or nothing (classic dictzip, whose last
		 * chunk carries the final block), then CRC-32 and ISIZE; applet/7dictzip.c:393-399 */
		unsigned char t[12];
		const size_t tn = fread(t, 1, 12, in);
		size_t at = 0;
		if (tn >= 10 && t[0] == 0x03 && t[1] == 0x00 && (tn == 10 || (tn == 12 && t[10] == 0x1f && t[11] == 0x8b)))
			at = 2;
		if (tn < at + 8) {
			fprintf(stderr, "unexpected end of file\n");
			ret = 1;
			goto out;
		}
		if (rd32(t + at) != fold.crc || rd32(t + at + 4) != (uint32_t)produced) {
			fprintf(stderr, "crc32 / size mismatch\n");
			ret = 1;
			goto out;
		}
		fseeko(in, -(long long)(tn - at - 8), SEEK_CUR);
	}
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(head);
	return ret;
}

int main(int argc, char **argv)
{
	struct hd_host_args a;
	hd_host_parse(&a, argc, argv, "X");
	if (a.bad || (a.decode && (a.n != 1 || a.level >= 0)) || (!a.decode && (a.n != 2 || a.level < 0 || a.level > 9))) {
		fprintf(stderr, "usage: %s -G<level> [-X] dec.bin enc.dz   or   -d enc.dz > dec.bin\n", argv[0]);
		return 1;
	}
	double t0;
	int ret = hd_host_begin(&t0);
	if (ret)
		return ret;
	FILE *in = fopen(a.name[0], "rb");
	if (!in) {
		fprintf(stderr, "failed to open %s\n", a.name[0]);
		return 2;
	}
	if (a.decode) {
		ret = dz_decompress(in, stdout);
	} else {
		FILE *out = fopen(a.name[1], "wb");
		if (!out) {
			fprintf(stderr, "failed to open %s\n", a.name[1]);
			fclose(in);
			return 3;
		}
		fprintf(stderr, "compression level = %d (hip)\n", a.level);
		ret = dz_compress(in, out, a.level, a.opt ? 0xff00 : 58315);
		if (fclose(out) && !ret)
			ret = 2;
	}
	fclose(in);
	return hd_host_end(t0, ret);
}
