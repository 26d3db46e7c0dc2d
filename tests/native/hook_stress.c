/*
 * hook_stress.c -- TEST ONLY: T threads x N calls of bgzf_compress() (bgzf_hook.c compiled with a sanitizer, linked
 * against stub_hipdeflate.c), every member checked against the block that went in; then the zlibutil_hip mirror
 * (hd_zlibutil_buffer_*) driven from threads the way applet/7bgzf.c:211 drives zlibutil_buffer_code; round 4: the codec
 * engines of the same batcher (hd_codec_batch) from the same T threads; then one engine of hd_call_batch.c under the
 * DECOMPRESS policy (what hip_inflate runs on, hd_api.hip) through a client made of two byte arenas.
 *   hook_stress [threads=64] [calls=10000]
 */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "hipdeflate.h"
#include "hd_call_batch.h"
#include "zlibutil_hip.h"

static int g_calls = 10000;
static int g_bad;

static void *worker(void *arg)
{
	const unsigned id = (unsigned)(uintptr_t)arg;
	unsigned char *src = (unsigned char *)malloc(0xff00), *dst = (unsigned char *)malloc(0x10000);
	unsigned seed = id * 2654435761u + 12345;
	for (int k = 0; k < g_calls; k++) {
		seed = seed * 1664525u + 1013904223u;
		const size_t n = (k % 97 == 0) ? 0 : 1 + (seed >> 8) % 0xff00;      /* now and then the EOF request */
		for (size_t i = 0; i < n; i += 61)
			src[i] = (unsigned char)(seed >> (i % 24));
		if (n) {
			src[n - 1] = (unsigned char)k;
			src[0] = (unsigned char)id;
		}
		size_t dlen = (k % 53 == 7) ? 20 : 0x10000;                          /* now and then too little room */
		const int r = bgzf_compress(dst, &dlen, src, n, -1);
		if (dlen == 20 && (k % 53 == 7)) {
			if (r != -1)
				__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
			continue;
		}
		if (r != 0 || (n == 0 && dlen != 28) ||
		    (n && (dlen != 18 + 5 + n + 8 || memcmp(dst + 23, src, n) || dst[23] != (unsigned char)id)))
			__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
	}
	free(src);
	free(dst);
	return NULL;
}

/* the per-block codecs' engines (bgzf_hook.c hd_codec_batch: one per level and raw frame), driven the same way; the stub's
 * contexts answer with the same stored BGZF-framed members whatever the frame */
int hd_codec_batch(unsigned char *dest, size_t *destLen, const unsigned char *src, size_t slen, int level, int flush);
static void *codec_worker(void *arg)
{
	const unsigned id = (unsigned)(uintptr_t)arg;
	unsigned char *src = (unsigned char *)malloc(0xff00), *dst = (unsigned char *)malloc(0x18000);
	unsigned seed = id * 2246822519u + 777;
	for (int k = 0; k < g_calls / 4 + 1; k++) {
		seed = seed * 1664525u + 1013904223u;
		const size_t n = 1 + (seed >> 8) % 0xff00;
		for (size_t i = 0; i < n; i += 61)
			src[i] = (unsigned char)(seed >> (i % 24));
		src[n - 1] = (unsigned char)k;
		src[0] = (unsigned char)id;
		size_t dlen = 0x18000;
		const int r = hd_codec_batch(dst, &dlen, src, n, 1 + (int)(id % 3), (int)(id & 1));
		if (r != 0 || dlen != 18 + 5 + n + 8 || memcmp(dst + 23, src, n) || dst[23] != (unsigned char)id)
			__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
	}
	if (hd_codec_batch(dst, &(size_t){ 0x18000 }, src, 0, 1, 0) != -2 || hd_codec_batch(dst, &(size_t){ 0x18000 }, src, 0x10000, 1, 0) != -2)
		__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);                   /* not for a batch: empty, or longer than a slot */
	free(src);
	free(dst);
	return NULL;
}

/* ---- the decompress policy: hip_inflate's client (hd_api.hip) restated over plain memory ------------------------------
 * A batch holds up to INF_SLOTS requests of one `flags` value in two arenas; a request takes up to a quarter of either, so
 * eight contexts hold as few as 32 of 64 callers (the wait for a free context), and a request the collecting batch has no
 * room for, or whose flags differ, closes it as it stands.  run() copies every request from the in-arena to the out-arena. */
#define INF_SLOTS 64
#define INF_ARENA 65536u
static struct inf_ctx {
	unsigned char in[INF_ARENA], out[INF_ARENA];
	uint32_t off_in[INF_SLOTS], off_out[INF_SLOTS], len[INF_SLOTS], flags_of[INF_SLOTS];
	uint32_t in_used, out_used, flags;
} g_ictx[HD_CB_CTX];
struct inf_req {
	uint32_t n, flags;
};
static int g_inf_runs_now, g_inf_runs_max, g_inf_batches;
#define BAD_IF(c) do { if (c) __atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED); } while (0)

static int inf_open(struct hd_cb *e, int k)
{
	(void)e;
	(void)k;
	static int once;                            /* the knobs, as hd_api.hip reads them: at the first open, before any leader looks */
	if (once++)
		return 0;
	const char *w;
	if ((w = getenv("HIPDEFLATE_INFLATE_WINDOW_US")))
		hd_cb_inflate.window_ns = atol(w) * 1000;
	if ((w = getenv("HIPDEFLATE_INFLATE_LINGER_US")))
		hd_cb_inflate.linger_ns = atol(w) * 1000;
	if ((w = getenv("HIPDEFLATE_INFLATE_INFLIGHT")) && atoi(w) >= 1)
		hd_cb_inflate.max_inflight = atoi(w);
	return 0;
}

static int inf_admit(struct hd_cb *e, int k, int idx, const void *req)
{
	(void)e;
	struct inf_ctx *c = &g_ictx[k];
	const struct inf_req *q = (const struct inf_req *)req;
	const uint32_t in_need = (q->n + 4 + 15) & ~15u, out_need = (q->n + 15) & ~15u;
	if (idx == 0) {
		c->in_used = c->out_used = 0;
		c->flags = q->flags;
	} else if (c->flags != q->flags || c->in_used + in_need > INF_ARENA || c->out_used + out_need > INF_ARENA) {
		return 0;
	}
	BAD_IF(idx >= INF_SLOTS);                   /* the policy closes a full batch */
	if (idx >= INF_SLOTS)
		abort();
	c->off_in[idx] = c->in_used;
	c->off_out[idx] = c->out_used;
	c->len[idx] = q->n;
	c->flags_of[idx] = q->flags;
	c->in_used += in_need;
	c->out_used += out_need;
	return 1;
}

static int inf_run(struct hd_cb *e, int k, int n)
{
	(void)e;
	struct inf_ctx *c = &g_ictx[k];
	const int now = __atomic_add_fetch(&g_inf_runs_now, 1, __ATOMIC_RELAXED);
	int max = __atomic_load_n(&g_inf_runs_max, __ATOMIC_RELAXED);
	while (now > max && !__atomic_compare_exchange_n(&g_inf_runs_max, &max, now, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED))
		;
	BAD_IF(now > HD_CB_CTX || n < 1 || n > INF_SLOTS || c->in_used > INF_ARENA || c->out_used > INF_ARENA);
	for (int i = 0; i < n; i++) {
		BAD_IF(c->flags_of[i] != c->flags || c->off_in[i] + c->len[i] > c->in_used || c->off_out[i] + c->len[i] > c->out_used);
		memcpy(c->out + c->off_out[i], c->in + c->off_in[i], c->len[i]);
	}
	/* every other batch stays out longer than a member spins: the members' sleep on the state word and the leader's wake */
	if (__atomic_add_fetch(&g_inf_batches, 1, __ATOMIC_RELAXED) & 1)
		nanosleep(&(struct timespec){ 0, 50000 }, NULL);
	__atomic_sub_fetch(&g_inf_runs_now, 1, __ATOMIC_RELAXED);
	return 0;
}

static void inf_close(struct hd_cb *e, int k)
{
	(void)e;
	(void)k;
}

static const struct hd_cb_client g_inf_client = { inf_open, inf_admit, inf_run, inf_close };
static struct hd_cb g_inf_eng = HD_CB_INIT(&g_inf_client, &hd_cb_inflate_policy, NULL, INF_SLOTS);

static void *inflate_policy_worker(void *arg)
{
	const unsigned id = (unsigned)(uintptr_t)arg;
	unsigned char *src = (unsigned char *)malloc(INF_ARENA / 4), *dst = (unsigned char *)malloc(INF_ARENA / 4);
	unsigned seed = id * 3266489917u + 4242;
	for (int k = 0; k < g_calls / 4 + 1; k++) {
		seed = seed * 1664525u + 1013904223u;
		/* 1 byte .. a quarter of the arena (less the 4 + 15 bytes of rounding the in-arena adds), most of them near it */
		const uint32_t top = INF_ARENA / 4 - 19;
		const uint32_t n = (seed >> 4) & 3 ? top - (seed >> 8) % 64 : 1 + (seed >> 8) % top;
		for (uint32_t i = 0; i < n; i += 61)
			src[i] = (unsigned char)(seed >> (i % 24));
		src[n - 1] = (unsigned char)k;
		src[0] = (unsigned char)id;
		memset(dst, 0xee, n);
		const struct inf_req q = { n, (seed >> 13) % 5 == 0 };
		struct hd_cb_seat s;
		if (hd_cb_join(&g_inf_eng, &q, &s) != 0) {
			__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
			continue;
		}
		struct inf_ctx *c = &g_ictx[s.k];
		memcpy(c->in + c->off_in[s.idx], src, n);
		const int rc = hd_cb_wait(&g_inf_eng, &s);
		memcpy(dst, c->out + c->off_out[s.idx], n);
		hd_cb_leave(&g_inf_eng, &s);
		BAD_IF(rc || memcmp(dst, src, n));
	}
	free(src);
	free(dst);
	return NULL;
}

static void *zlibutil_worker(void *arg)
{
	const unsigned id = (unsigned)(uintptr_t)arg;
	for (int k = 0; k < 200; k++) {
		hd_zlibutil_buffer *zb = hd_zlibutil_buffer_allocate(6000, 4000 + id);
		if (!zb) {
			__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
			continue;
		}
		memset(zb->source, (int)(id + k), zb->sourceLen);
		zb->func = (void *)hip_deflate;
		zb->encode = 1;
		zb->level = 1;
		zb->rfc1952 = k & 1;
		zb->rfc1950 = !(k & 1) && (k & 2);
		hd_zlibutil_buffer_code(zb);
		if (zb->ret || zb->destLen < zb->sourceLen)
			__atomic_add_fetch(&g_bad, 1, __ATOMIC_RELAXED);
		hd_zlibutil_buffer_free(zb);
	}
	return NULL;
}

int main(int argc, char **argv)
{
	const int T = argc > 1 ? atoi(argv[1]) : 64;
	if (argc > 2)
		g_calls = atoi(argv[2]);
	pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)(T > 8 ? T : 8));
	for (int i = 0; i < T; i++)
		pthread_create(&th[i], NULL, worker, (void *)(uintptr_t)i);
	for (int i = 0; i < T; i++)
		pthread_join(th[i], NULL);
	for (int i = 0; i < T; i++)
		pthread_create(&th[i], NULL, codec_worker, (void *)(uintptr_t)i);
	for (int i = 0; i < T; i++)
		pthread_join(th[i], NULL);
	/* the decompress policy from 64 threads whatever T is (the wait for a free context needs them), then alone: the policy
	 * remembers the 64 and must let go of them, a lone caller's batches close on the linger time meanwhile */
	pthread_t ith[64];
	for (int i = 0; i < 64; i++)
		pthread_create(&ith[i], NULL, inflate_policy_worker, (void *)(uintptr_t)i);
	for (int i = 0; i < 64; i++)
		pthread_join(ith[i], NULL);
	const int before = g_inf_batches, calls = g_calls;
	g_calls = 4 * 200 - 4;
	inflate_policy_worker((void *)(uintptr_t)64);
	g_calls = calls;
	if (g_inf_batches - before != 200 || g_inf_eng.active || g_inf_eng.running || g_inf_eng.inflight || g_inf_eng.open != -1)
		g_bad++;
	hd_cb_drain(&g_inf_eng);
	printf("hook_stress: decompress policy: %d batches, %d side by side at most\n", g_inf_batches, g_inf_runs_max);
	for (int i = 0; i < 8; i++)
		pthread_create(&th[i], NULL, zlibutil_worker, (void *)(uintptr_t)i);
	for (int i = 0; i < 8; i++)
		pthread_join(th[i], NULL);
	free(th);
	printf("hook_stress: %d threads x %d calls, %d bad\n", T, g_calls, g_bad);
	return g_bad ? 1 : 0;
}
