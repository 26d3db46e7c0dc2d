/*
 * hd_razf_host.c -- hd7razf: applet/7razf.c (_compress :160-304, _decompress
 * :306-383) over libhipdeflate.so.  RAZF is the random-access gzip of old samtools:
 * ONE gzip member with an 'RAZF' extra field, 32 KiB chunks of which every one but
 * the last ends in a full flush (the last is an ordinary final stream), CRC-32 and
 * ISIZE, then a big-endian index (chunk count - 1, 64-bit bin offsets every 2^32
 * input bytes, 32-bit chunk offsets inside the bin) and two 64-bit totals.
 *
 *     hd7razf -G<level> dec.bin > enc.raz
 *     hd7razf -d enc.raz > dec.bin
 *
 * What changed, and why: as hd7dictzip -- chunks go to the device in batches and
 * leave in full-flush form (HD_FRAME_RAW_FLUSH; the last chunk HD_FRAME_RAW), no
 * re-inflate on the CPU (zlibutil_buffer_full_flush, applet/7razf.c:126-160), the
 * member CRC-32 is folded from the kernel's per-chunk CRCs, and the reader checks
 * CRC-32 and size, which the reference's does not.  The first chunk has index -1
 * and no cell in the table, as there (:177,:277).
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hd_host_batch.h"

#define RZ_BLOCK 32768u
#define RZ_BATCH 4096                 /* chunks per device call */
#define RZ_BINSIZE ((1ull << 32) / RZ_BLOCK)

static const unsigned char rz_header[19] = { 0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0x03, 0x07, 0x00,
					     'R',  'A',  'Z',  'F',  0x01, 0x80, 0x00 };

static int rz_compress(FILE *in, FILE *out, int level)
{
	const long long total = file_size(in);
	if (total <= 0) {
		fprintf(stderr, total ? "cannot stat the input\n" : "empty input\n");
		return 2;
	}
	const long long nchunks = (total + RZ_BLOCK - 1) / RZ_BLOCK;
	const long long total_block = nchunks - 1;          /* the reference's count: chunk -1 is not indexed */
	const long long bins = total_block / (long long)RZ_BINSIZE;
	const size_t index_bytes = 4 + 8 * (size_t)(bins + 1) + 4 * (size_t)total_block;
	struct hd_batch b;
	int ret = hd_batch_open(&b, RZ_BATCH, (size_t)RZ_BATCH * RZ_BLOCK, up16(RZ_BLOCK + 5 * 2 + 32), 1);
	unsigned char *index = calloc(1, index_bytes + 16);
	if (!ret && !index) {
		fprintf(stderr, "out of memory\n");
		ret = 2;
	}
	if (ret)
		goto out;
	unsigned char *bin_tab = index + 4, *cell_tab = index + 4 + 8 * (size_t)(bins + 1);
	wr32be(index, (uint32_t)total_block);
	fwrite(rz_header, 1, sizeof(rz_header), out);
	uint64_t pos = sizeof(rz_header);
	struct crc_fold fold = { 0, 0, 0 };
	long long left = total;
	for (long long c = 0; c < nchunks; c += RZ_BATCH) {
		const uint32_t n = (uint32_t)(nchunks - c < RZ_BATCH ? nchunks - c : RZ_BATCH);
		/* every chunk but the file's last in full-flush form; the last one is a finished stream (:226-236) */
		if ((ret = hd_batch_read(&b, in, n, RZ_BLOCK, &left)) ||
		    (ret = hd_batch_deflate(&b, n, level, HD_FRAME_RAW_FLUSH, c + n == nchunks ? HD_FRAME_RAW : HD_FRAME_RAW_FLUSH)))
			goto out;
		for (uint32_t i = 0; i < n; i++) {
			const long long idx = c + i - 1;      /* the reference's i: -1 for the first chunk */
			if (idx >= 0) {
				if (idx % (long long)RZ_BINSIZE == 0)
					wr64be(bin_tab + 8 * (size_t)(idx / (long long)RZ_BINSIZE), pos);
				wr32be(cell_tab + 4 * (size_t)idx, (uint32_t)(pos - rd64be(bin_tab + 8 * (size_t)(idx / (long long)RZ_BINSIZE))));
			}
			fwrite(b.out + (size_t)i * b.stride, 1, b.olen[i], out);
			pos += b.olen[i];
			crc_append(&fold, b.crc[i], b.len[i]);
		}
		fprintf(stderr, "%lld / %lld\r", c + n - 1, total_block);
	}
	unsigned char t[16];
	wr32(t, fold.crc);
	wr32(t + 4, (uint32_t)total);
	fwrite(t, 1, 8, out);
	pos += 8;
	fwrite(index, 1, index_bytes, out);
	wr64be(t, (uint64_t)total);
	wr64be(t + 8, pos);                                 /* where the index starts */
	fwrite(t, 1, 16, out);
	fprintf(stderr, "%lld / %lld done.\n", total_block, total_block);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(index);
	return ret;
}

static int rz_decompress(FILE *in, FILE *out)
{
	unsigned char head[64], tail[16];
	const long long fsize = file_size(in);
	if (fread(head, 1, 19, in) != 19 || memcmp(head, rz_header, 4) || !(head[3] & 4) || rd16(head + 10) < 7 ||
	    memcmp(head + 12, "RAZF", 4)) {
		fprintf(stderr, "not RAZF\n");
		return 1;
	}
	const uint32_t block_size = (head[17] << 8) | head[18];
	const size_t hdr_len = 12 + rd16(head + 10);
	if (!block_size || fsize < (long long)hdr_len + 8 + 4 + 8 + 16 || fseeko(in, -16, SEEK_END)) {
		fprintf(stderr, "input is not seekable or truncated\n");
		return 1;
	}
	if (fread(tail, 1, 16, in) != 16)
		return 1;
	const uint64_t total_bytes = rd64be(tail), index_at = rd64be(tail + 8);
	if (index_at + 4 + 8 + 16 > (uint64_t)fsize || index_at < hdr_len + 8 || fseeko(in, (long long)index_at, SEEK_SET) ||
	    fread(head + 32, 1, 4, in) != 4) {
		fprintf(stderr, "corrupted index\n");
		return 1;
	}
	const long long total_block = (int32_t)rd32be(head + 32);
	const uint64_t binsize = (1ull << 32) / block_size;
	const long long bins = total_block / (long long)binsize;
	const size_t tab_bytes = 8 * (size_t)(bins + 1) + 4 * (size_t)total_block;
	if (total_block < 0 || index_at + 4 + tab_bytes + 16 != (uint64_t)fsize) {
		fprintf(stderr, "corrupted index\n");
		return 1;
	}
	struct hd_batch b;
	int ret = hd_batch_open(&b, RZ_BATCH, 0, up16(block_size), 1);
	unsigned char *tab = malloc(tab_bytes + 16);
	if (ret)
		goto out;
	if (!tab || fread(tab, 1, tab_bytes, in) != tab_bytes) {
		fprintf(stderr, "corrupted index\n");
		ret = 1;
		goto out;
	}
	const unsigned char *cell_tab = tab + 8 * (size_t)(bins + 1);
	const long long nchunks = total_block + 1;
	/* start of chunk k (k = the reference's i + 1); chunk nchunks "starts" at the trailer's end (:325) */
#define RZ_START(k) ((k) == 0 ? (uint64_t)hdr_len : (k) == nchunks ? index_at : \
		     rd64be(tab + 8 * (size_t)(((k) - 1) / (long long)binsize)) + rd32be(cell_tab + 4 * (size_t)((k) - 1)))
	struct crc_fold fold = { 0, 0, 0 };
	uint64_t produced = 0;
	for (long long c = 0; c < nchunks; c += RZ_BATCH) {
		const uint32_t m = (uint32_t)(nchunks - c < RZ_BATCH ? nchunks - c : RZ_BATCH);
		const uint64_t first = RZ_START(c), end = RZ_START(c + m);
		if (end < first || end > index_at) {
			fprintf(stderr, "corrupted index\n");
			ret = 1;
			goto out;
		}
		const size_t itotal = (size_t)(end - first);
		if ((ret = hd_grow(&b.in, &b.icap, itotal)))
			goto out;
		if (fseeko(in, (long long)first, SEEK_SET) || fread(b.in, 1, itotal, in) != itotal) {
			fprintf(stderr, "unexpected end of file\n");
			ret = 1;
			goto out;
		}
		for (uint32_t i = 0; i < m && !ret; i++) {
			const uint64_t lo = RZ_START(c + i), hi = RZ_START(c + i + 1);
			if (lo < first || hi < lo || hi > end)
				ret = 1;
			b.off[i] = lo - first;
			b.len[i] = (uint32_t)(hi - lo);        /* the last chunk's span takes the 8 trailer bytes along, as there */
			b.ooff[i] = (uint64_t)i * b.stride;
			b.cap[i] = block_size;
		}
		if (ret) {
			fprintf(stderr, "corrupted index\n");
			goto out;
		}
		if ((ret = hd_batch_inflate(&b, m, 1)))
			goto out;
		for (uint32_t i = 0; i < m; i++) {
			fwrite(b.out + b.ooff[i], 1, b.olen[i], out);
			crc_append(&fold, b.crc[i], b.olen[i]);
			produced += b.olen[i];
		}
		fprintf(stderr, "%lld / %lld\r", c + m - 1, total_block);
	}
#undef RZ_START
	fprintf(stderr, "%lld / %lld done.\n", total_block, total_block);
	unsigned char t[8];
	if (fseeko(in, (long long)index_at - 8, SEEK_SET) || fread(t, 1, 8, in) != 8 || rd32(t) != fold.crc ||
	    rd32(t + 4) != (uint32_t)produced || produced != total_bytes) {
		fprintf(stderr, "crc32 / size mismatch\n");
		ret = 1;
	} else if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(tab);
	return ret;
}

int main(int argc, char **argv)
{
	struct hd_host_args a;
	hd_host_parse(&a, argc, argv, NULL);
	if (a.bad || a.n != 1 || (a.decode && a.level >= 0) || (!a.decode && (a.level < 0 || a.level > 9))) {
		fprintf(stderr, "usage: %s -G<level> dec.bin > enc.raz   or   -d enc.raz > dec.bin\n", argv[0]);
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
		ret = rz_decompress(in, stdout);
	} else {
		fprintf(stderr, "compression level = %d (hip)\n", a.level);
		ret = rz_compress(in, stdout, a.level);
	}
	fclose(in);
	return hd_host_end(t0, ret);
}
