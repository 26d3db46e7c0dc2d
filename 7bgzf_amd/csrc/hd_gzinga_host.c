/*
 * hd_gzinga_host.c -- hd7gzinga: applet/7gzinga.c (_compress :77-197, _decompress
 * :199-305) over libhipdeflate.so.  GZinga is a seekable / splittable gzip: every
 * 100 KiB block is its own member whose header carries an (empty) comment, and a
 * last member with no data holds the index as ITS comment: "k:<end offset of block
 * k>;" for every block.
 *
 *     hd7gzinga -G<level> < dec.bin > enc.gz
 *     hd7gzinga -d enc.gz > dec.bin
 *
 * What changed, and why: blocks go to the device in batches (HD_FRAME_RAW; CRC-32 of
 * each block comes back with it, so there is no fcrc32 pass on the host, :176) and
 * the reader hands whole runs of members to one batched inflate, checking CRC-32
 * and ISIZE of every member (the reference checks neither).  The reference reads
 * the index from the last 32 KiB of the file only (:212-216), which bounds ITS
 * reader to about 2,500 blocks; this reader widens the search until it finds the
 * index member.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include "hd_host_batch.h"

#define GZ_BLOCK (100u * 1024u)
#define GZ_BATCH 1024
#define GZ_MAX_ISIZE (64u << 20)      /* a member claiming more than this is not ours nor the reference's */

static const unsigned char gz_header[9] = { 0x1f, 0x8b, 0x08, 0x10, 0, 0, 0, 0, 0x00 };

static int gz_compress(FILE *in, FILE *out, int level)
{
	uint64_t *ends = NULL;
	size_t nends = 0, cap_ends = 0;
	struct hd_batch b;
	int ret = hd_batch_open(&b, GZ_BATCH, (size_t)GZ_BATCH * GZ_BLOCK, up16(GZ_BLOCK + 5 * 3 + 32), 1);
	if (ret)
		goto out;
	uint64_t total_size = 0;
	for (;;) {
		const size_t got = read_full(in, b.in, (size_t)GZ_BATCH * GZ_BLOCK);
		if (!got)
			break;
		const uint32_t n = (uint32_t)((got + GZ_BLOCK - 1) / GZ_BLOCK);
		hd_batch_split(&b, n, GZ_BLOCK, got);
		if ((ret = hd_batch_deflate(&b, n, level, HD_FRAME_RAW, HD_FRAME_RAW)))
			goto out;
		if (nends + n > cap_ends) {
			uint64_t *e = realloc(ends, (nends + n) * 2 * sizeof(uint64_t));
			if (!e) {
				fprintf(stderr, "out of memory\n");
				ret = 2;
				goto out;
			}
			ends = e, cap_ends = (nends + n) * 2;
		}
		for (uint32_t i = 0; i < n; i++) {
			unsigned char t[11];
			memcpy(t, gz_header, 9);
			t[9] = 0xff, t[10] = 0x00;                /* OS = unknown, then the empty comment */
			fwrite(t, 1, 11, out);
			fwrite(b.out + (size_t)i * b.stride, 1, b.olen[i], out);
			wr32(t, b.crc[i]);
			wr32(t + 4, b.len[i]);
			fwrite(t, 1, 8, out);
			total_size += 11 + (uint64_t)b.olen[i] + 8;
			ends[nends++] = total_size;
		}
		fprintf(stderr, "%zu\r", nends);
		if (got < (size_t)GZ_BATCH * GZ_BLOCK)
			break;
	}
	unsigned char t[11] = { 0x1f, 0x8b, 0x08, 0x10, 0, 0, 0, 0, 0x00, 0xff };
	fwrite(t, 1, 10, out);
	for (size_t k = 0; k < nends; k++)
		fprintf(out, "%zu:%llu;", k, (unsigned long long)ends[k]);
	memset(t, 0, sizeof(t));
	t[1] = 0x03;                                          /* NUL ends the comment; 03 00 = empty final block; CRC 0, ISIZE 0 */
	fwrite(t, 1, 11, out);
	fprintf(stderr, "%zu done.\n", nends);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(ends);
	return ret;
}

/* read_gz_header_generic's job: length of a gzip member header, 0 if it is none */
static size_t gz_member_header(const unsigned char *d, size_t size)
{
	if (size < 10 || d[0] != 0x1f || d[1] != 0x8b || d[2] != 8 || (d[3] & 0xe0))
		return 0;
	size_t n = 10;
	if (d[3] & 4) {
		if (size < n + 2)
			return 0;
		n += 2 + rd16(d + n);
	}
	if (d[3] & 8) {
		while (n < size && d[n])
			n++;
		n++;
	}
	if (d[3] & 16) {
		while (n < size && d[n])
			n++;
		n++;
	}
	if (d[3] & 2)
		n += 2;
	return n <= size ? n : 0;
}

static int gz_decompress(FILE *in, FILE *out)
{
	const long long fsize = file_size(in);
	if (fsize < 21) {
		fprintf(stderr, "not GZinga or corrupted\n");
		return 1;
	}
	unsigned char *foot = NULL;
	uint64_t *lst = NULL;
	struct hd_batch b;
	int ret = hd_batch_open(&b, GZ_BATCH, 0, 0, 1);
	if (ret)
		goto out;
	/* the index member is the last place the 9 header bytes occur (:217-227) */
	size_t foot_len = 0;
	long long index_at = -1;
	for (size_t span = 32 * 1024;; span *= 4) {
		if ((long long)span > fsize)
			span = (size_t)fsize;
		free(foot);
		foot = malloc(span + 1);
		if (!foot || fseeko(in, fsize - (long long)span, SEEK_SET) || read_full(in, foot, span) != span) {
			fprintf(stderr, "cannot read the index\n");
			ret = 1;
			goto out;
		}
		foot_len = span;
		foot[span] = 0;
		/* an index is text: it cannot itself contain the header bytes, so the last occurrence whose comment
		 * runs to the file's final 11 bytes is the index member */
		for (size_t k = span >= 9 ? span - 9 + 1 : 0; k-- > 0;) {
			if (!memcmp(foot + k, gz_header, 9)) {
				const size_t text = k + 10;
				const size_t nul = text + strlen((const char *)foot + text);
				if (nul + 11 == span)
					index_at = fsize - (long long)span + (long long)k;
				break;
			}
		}
		if (index_at >= 0 || (long long)span == fsize)
			break;
	}
	if (index_at < 0) {
		fprintf(stderr, "not GZinga or corrupted\n");
		ret = 1;
		goto out;
	}
	/* "k:<end>;" ... */
	const char *p = (const char *)foot + (size_t)(index_at - (fsize - (long long)foot_len)) + 10;
	size_t nblk = 0, cap_lst = 2;
	lst = malloc(sizeof(uint64_t) * cap_lst);
	if (lst)
		lst[0] = 0;
	while (lst && *p) {
		char *e;
		(void)strtoull(p, &e, 10);
		if (e == p || *e != ':') {
			ret = 1;
			break;
		}
		p = e + 1;
		const uint64_t v = strtoull(p, &e, 10);
		if (e == p || *e != ';' || v < lst[nblk] + 19 || v > (uint64_t)index_at) {
			ret = 1;
			break;
		}
		p = e + 1;
		if (nblk + 2 > cap_lst) {
			uint64_t *l = realloc(lst, sizeof(uint64_t) * cap_lst * 2);
			if (!l) {
				ret = 1;
				break;
			}
			lst = l, cap_lst *= 2;
		}
		lst[++nblk] = v;
	}
	free(foot);
	foot = NULL;
	if (!lst || ret || (nblk ? lst[nblk] : 0) != (uint64_t)index_at) {
		fprintf(stderr, "corrupted index\n");
		ret = 1;
		goto out;
	}
	for (size_t c = 0; c < nblk; c += GZ_BATCH) {
		const uint32_t m = (uint32_t)(nblk - c < GZ_BATCH ? nblk - c : GZ_BATCH);
		const size_t itotal = (size_t)(lst[c + m] - lst[c]);
		if (hd_grow(&b.in, &b.icap, itotal) || fseeko(in, (long long)lst[c], SEEK_SET) || read_full(in, b.in, itotal) != itotal) {
			fprintf(stderr, "file truncated\n");
			ret = 1;
			goto out;
		}
		size_t ototal = 0;
		for (uint32_t i = 0; i < m; i++) {
			const size_t a = (size_t)(lst[c + i] - lst[c]), mlen = (size_t)(lst[c + i + 1] - lst[c + i]);
			const size_t n = gz_member_header(b.in + a, mlen);
			if (!n || n + 8 > mlen || rd32(b.in + a + mlen - 4) > GZ_MAX_ISIZE) {
				fprintf(stderr, "corrupted\n");
				ret = 1;
				goto out;
			}
			b.off[i] = a + n;
			b.len[i] = (uint32_t)(mlen - n - 8);
			b.cap[i] = rd32(b.in + a + mlen - 4);
			b.ooff[i] = ototal;
			ototal += up16(b.cap[i]);
		}
		if ((ret = hd_grow(&b.out, &b.ocap, ototal)) || (ret = hd_batch_inflate(&b, m, 0)))
			goto out;
		for (uint32_t i = 0; i < m; i++) {
			/* the member's CRC-32 sits 8 bytes before its end */
			if (b.olen[i] != b.cap[i] || b.crc[i] != rd32(b.in + (size_t)(lst[c + i + 1] - lst[c]) - 8)) {
				fprintf(stderr, "crc32 / size mismatch\n");
				ret = 1;
				goto out;
			}
			fwrite(b.out + b.ooff[i], 1, b.olen[i], out);
		}
		fprintf(stderr, "%zu\r", c + m);
	}
	fprintf(stderr, "%zu done.\n", nblk);
	if (fflush(out) || ferror(out)) {
		fprintf(stderr, "write error\n");
		ret = 2;
	}
out:
	hd_batch_close(&b);
	free(foot);
	free(lst);
	return ret;
}

int main(int argc, char **argv)
{
	struct hd_host_args a;
	hd_host_parse(&a, argc, argv, NULL);
	if (a.bad || (a.decode && (a.n != 1 || a.level >= 0)) || (!a.decode && (a.n || a.level < 0 || a.level > 9)) ||
	    (!a.decode && (isatty(0) || isatty(1)))) {
		fprintf(stderr, "usage: %s -G<level> < dec.bin > enc.gz   or   -d enc.gz > dec.bin\n", argv[0]);
		return 1;
	}
	double t0;
	int ret = hd_host_begin(&t0);
	if (ret)
		return ret;
	if (a.decode) {
		FILE *in = fopen(a.name[0], "rb");
		if (!in) {
			fprintf(stderr, "failed to open %s\n", a.name[0]);
			return 2;
		}
		ret = gz_decompress(in, stdout);
		fclose(in);
	} else {
		fprintf(stderr, "compression level = %d (hip)\n", a.level);
		ret = gz_compress(stdin, stdout, a.level);
	}
	return hd_host_end(t0, ret);
}
