/*
 * hd_host_batch.h -- the scaffolding the chunked container hosts (hd7dictzip, hd7razf, hd7gzinga, hd7ciso,
 * hd7daxcr) share: the host buffers and per-chunk arrays of one device batch, the batch calls with their status
 * checks, and the front end of main() (-d -c -@N -G<l>/-l<l> and names; init, timer, shutdown).  What a format
 * does with the results -- index cells, sector tables, thresholds, trailers -- stays in the format's own file.
 * Header-only: each host is one translation unit.
 */
#ifndef HD_HOST_BATCH_H
#define HD_HOST_BATCH_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hipdeflate.h"
#include "hd_host_util.h"

/* One batch.  Deflate: chunk i is in[off[i] .. +len[i]), its output out + i * stride.  Inflate: off/len are the
 * input spans, ooff/cap the output slots.  olen, crc (NULL unless asked for) and st come back from the device. */
struct hd_batch {
	unsigned char *in, *out;
	size_t icap, ocap;            /* bytes behind in / out, 16 of them slack */
	uint64_t stride;
	uint64_t *off, *ooff;
	uint32_t *len, *cap, *olen, *crc;
	int32_t *st;
};

/* free(*buf) and allocate need + 16 bytes if *cap is short of that; 2 ("out of memory") on failure */
static inline int hd_grow(unsigned char **buf, size_t *cap, size_t need)
{
	if (need + 16 <= *cap && *buf)
		return 0;
	free(*buf);
	*buf = malloc(*cap = need + 16);
	if (*buf)
		return 0;
	*cap = 0;
	fprintf(stderr, "out of memory\n");
	return 2;
}

static inline void hd_batch_close(struct hd_batch *b)
{
	free(b->in), free(b->out), free(b->off), free(b->ooff), free(b->len), free(b->cap), free(b->olen), free(b->crc),
		free(b->st);
	*b = (struct hd_batch){ 0 };
}

/* Arrays for max_chunks chunks; in_bytes of input and max_chunks * out_stride of output now unless 0 (then
 * hd_grow them per batch).  2 ("out of memory") on failure; hd_batch_close is safe on what is open either way. */
static inline int hd_batch_open(struct hd_batch *b, uint32_t max_chunks, size_t in_bytes, uint64_t out_stride, int with_crc)
{
	*b = (struct hd_batch){ .stride = out_stride };
	b->off = malloc(sizeof(uint64_t) * max_chunks), b->ooff = malloc(sizeof(uint64_t) * max_chunks);
	b->len = malloc(sizeof(uint32_t) * max_chunks), b->cap = malloc(sizeof(uint32_t) * max_chunks);
	b->olen = malloc(sizeof(uint32_t) * max_chunks), b->st = malloc(sizeof(int32_t) * max_chunks);
	if (with_crc)
		b->crc = malloc(sizeof(uint32_t) * max_chunks);
	if (!b->off || !b->ooff || !b->len || !b->cap || !b->olen || !b->st || (with_crc && !b->crc)) {
		fprintf(stderr, "out of memory\n");
		return 2;
	}
	if (in_bytes && hd_grow(&b->in, &b->icap, in_bytes))
		return 2;
	return out_stride ? hd_grow(&b->out, &b->ocap, (size_t)max_chunks * out_stride) : 0;
}

/* chunks 0..n-1 of b->in: `block` bytes each, bytes in all (the last may be short) */
static inline void hd_batch_split(struct hd_batch *b, uint32_t n, uint32_t block, size_t bytes)
{
	for (uint32_t i = 0; i < n; i++) {
		b->off[i] = (uint64_t)i * block;
		b->len[i] = bytes - b->off[i] < block ? (uint32_t)(bytes - b->off[i]) : block;
	}
}

/* the next n chunks of `block` bytes (*left bytes remain in the input) into b->in; 2 on a short read */
static inline int hd_batch_read(struct hd_batch *b, FILE *in, uint32_t n, uint32_t block, long long *left)
{
	const size_t want = *left < (long long)n * block ? (size_t)*left : (size_t)n * block;
	if (fread(b->in, 1, want, in) != want) {
		fprintf(stderr, "short read\n");
		return 2;
	}
	*left -= (long long)want;
	hd_batch_split(b, n, block, want);
	return 0;
}

/* Encode chunks 0..n-1 of b->in in `frame`; if last_frame differs, chunk n-1 goes alone in last_frame.  1 on a
 * failed call or chunk ("hip_deflate %d"). */
static inline int hd_batch_deflate(struct hd_batch *b, uint32_t n, int level, int frame, int last_frame)
{
	const uint32_t k = last_frame != frame ? n - 1 : n;
	const uint32_t cap = (uint32_t)b->stride;
	int r = 0;
	if (k)
		r = hipdeflate_batch_deflate(b->in, b->off, b->len, k, level, frame, b->out, b->stride, cap, b->olen, b->crc, b->st);
	if (!r && k < n)
		r = hipdeflate_batch_deflate(b->in, b->off + k, b->len + k, 1, level, last_frame, b->out + (size_t)k * b->stride,
					     b->stride, cap, b->olen + k, b->crc ? b->crc + k : NULL, b->st + k);
	for (uint32_t i = 0; i < n && !r; i++)
		r = b->st[i];
	if (r) {
		fprintf(stderr, "hip_deflate %d\n", r);
		return 1;
	}
	return 0;
}

/* Decode streams 0..m-1 (hipdeflate_batch_inflate_flush's stopping rule if flushed).  1 on a failed call or
 * stream ("inflate %d"). */
static inline int hd_batch_inflate(struct hd_batch *b, uint32_t m, int flushed)
{
	if (!m)
		return 0;
	int r = (flushed ? hipdeflate_batch_inflate_flush : hipdeflate_batch_inflate)(b->in, b->off, b->len, m, b->out, b->ooff,
										       b->cap, b->olen, b->crc, b->st);
	for (uint32_t i = 0; i < m && !r; i++)
		r = b->st[i];
	if (r) {
		fprintf(stderr, "inflate %d\n", r);
		return 1;
	}
	return 0;
}

/* ---- main() ------------------------------------------------------------------------------------------------------ */

struct hd_host_args {
	int decode, level, bad, n;    /* level -1: none given; n: names given (a third one sets bad) */
	const char *name[2];
	const char *opt;              /* the host's own option: what follows its letter, NULL if absent */
};

/* -d, -c (ignored), -@<threads> (ignored), -G<level> / -l<level>, and the host's own option `own`: a letter, with
 * ':' after it if it takes the rest of the argument as its value (getopt's convention).  Anything else sets bad. */
static inline void hd_host_parse(struct hd_host_args *a, int argc, char **argv, const char *own)
{
	*a = (struct hd_host_args){ .level = -1 };
	for (int i = 1; i < argc; i++) {
		const char *s = argv[i];
		if (s[0] != '-' || !s[1]) {
			if (a->n < 2)
				a->name[a->n++] = s;
			else
				a->bad = 1;
			continue;
		}
		for (const char *p = s + 1; *p; p++) {
			if (*p == 'd') {
				a->decode = 1;
			} else if (*p == 'c') {
			} else if (*p == '@') {
				break;
			} else if (*p == 'G' || *p == 'l') {
				a->level = p[1] ? atoi(p + 1) : 1;
				break;
			} else if (own && *own == *p) {
				a->opt = p + 1;
				if (own[1] == ':')
					break;
			} else {
				a->bad = 1;
				break;
			}
		}
	}
}

/* hipdeflate_init(-1) and the clock; 4, the exit code, with the message if there is no usable device */
static inline int hd_host_begin(double *t0)
{
	const int r = hipdeflate_init(-1);
	if (r) {
		fprintf(stderr, "hipdeflate: no usable device (%d): %s\n", r, hipdeflate_version());
		return 4;
	}
	*t0 = now_s();
	return 0;
}

static inline int hd_host_end(double t0, int ret)
{
	fprintf(stderr, "ellapsed time: %.3f sec\n", now_s() - t0);
	hipdeflate_shutdown();
	return ret;
}

#endif
