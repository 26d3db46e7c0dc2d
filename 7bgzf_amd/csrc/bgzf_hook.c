/*
 * bgzf_hook.c -- the LD_PRELOAD hook: BGZF_METHOD=hip<level> LD_PRELOAD=./libhipdeflate.so samtools ...
 *
 * Same exported symbol, signature and return values as the reference's
 * bgzf_compress (bgzf_compress.c:39-198): htslib's own bgzf_compress is
 * shadowed through the PLT, so samtools/bcftools must link libhts.so
 * (readme.md:9-14).  Differences, all forced by the device:
 *
 *  - The only coder here is "hip" (BGZF_METHOD=hip, hip1 ... hip9; the trailing
 *    digits are the level, parsed as bgzf_compress.c:60-70 does; no digits = level 1,
 *    hip's default as each method has one at :102-112).  BGZF_METHOD unset or empty
 *    is the reference's default, its zlib at level 6 (:54,:102), i.e. hip6: whoever
 *    preloads this library in place of the reference's gets the bytes-per-block class
 *    he had (until late in round 3 the answer was hip1, 0.45 of the input where zlib-6 makes 0.26;
 *    hip6 makes 0.277).  A BGZF_METHOD that
 *    names one of the reference's CPU coders, or an unknown name (which the reference
 *    silently runs as zlib, :54), keeps WRITING: the hip coder runs at the level the
 *    reference would have used for that name -- its digits, else the method's default
 *    of :102-112 (zlib / libdeflate / zlibng / cryptopp / unknown 6, 7zip 2, the others
 *    1), cut to 9 -- and one line on stderr says so.  (Rounds 1-2 returned -1, "coder
 *    missing", for such names: a user with BGZF_METHOD=libdeflate6 left in the
 *    environment got failing writes where the reference compresses.)
 *  - htslib calls the hook once per 0xff00-byte block from each of its worker
 *    threads and waits for the member.  Calls that arrive together share one
 *    latency-mode batch (hipdeflate_lat_*, HD_FRAME_LATENCY: 16 wavefronts per block
 *    at level 1, members framed by the kernel: header, BSIZE, CRC32, ISIZE, i.e.
 *    bgzf_compress.c:191-197).  Every caller copies its own block into the batch's
 *    pinned memory and its own member out of it, outside any lock; the first caller
 *    of a batch (its leader) waits until every caller that is inside the hook and not
 *    in a batch on the device has joined, nobody has joined for HIPDEFLATE_LINGER_US
 *    (8) or HIPDEFLATE_BATCH_US microseconds (default 60) have passed, launches, and
 *    publishes the result; the others spin on the batch's state (HIPDEFLATE_SPIN_US,
 *    default 400, then they sleep on that word; with more callers than cores they sleep at once).  HD_CB_CTX batches can be in flight at once (one
 *    collecting, the others on the device).  A lone caller does not wait at all.
 *    That protocol and its policy are hd_call_batch.c's; this file is its client.
 */
#define _GNU_SOURCE
#include <limits.h>
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <unistd.h>
#include "hipdeflate.h"
#include "hipdeflate_params.h"
#include "hd_call_batch.h"

#define HOOK_MAX_BATCH 256
#define HOOK_BLOCK 0xff00u           /* what a latency-mode BGZF slot takes (16 x 4080); htslib's BGZF_BLOCK_SIZE */

/* HIPDEFLATE_HOOK_STATS=1: where the time of a call goes, printed at exit (tools/hook_bench.c reads it) */
static struct hd_cb_stats g_st;

/* One ENGINE per (level, frame): the hook's (BGZF members at BGZF_METHOD's level) and, since round 4, one per level and raw
 * frame for the per-block codecs -- hip_deflate / hip_deflate_flush called from the reference's -@N threads
 * (applet/7bgzf.c:211) share launches exactly as htslib's workers do in the hook (16 callers: 3.8 -> 8.6 GB/s at level 1,
 * and 64 callers no longer collapse to 1.2).  The batching itself is hd_call_batch.c's, under its compress policy; what a
 * batch owns here is a latency context: input slot idx, hipdeflate_lat_run, output slot idx. */
struct hook_eng {
	struct hd_cb cb;             /* (first: the client's functions get it back as their engine) */
	hipdeflate_lat *lat[HD_CB_CTX];
	uint32_t len[HD_CB_CTX][HOOK_MAX_BATCH];
	int level, frame;            /* level: the hook's (BGZF_METHOD; a codec engine's is its index); frame: HD_FRAME_BGZF, HD_FRAME_RAW or HD_FRAME_RAW_FLUSH */
	int loud;                    /* the hook prints codec errors as the reference does (bgzf_compress.c:163-169) */
};

/* ---- the engine's client: a batch context is a latency context ----------------------------------------------------- */
static int hook_open(struct hd_cb *cb, int k)
{
	struct hook_eng *e = (struct hook_eng *)cb;
	/* batch context k lives on entry k of the device list (HIPDEFLATE_DEVICES), round robin */
	const int ndev = hipdeflate_device_count();
	e->lat[k] = hipdeflate_lat_open_on(ndev > 0 ? k % ndev : 0, e->level, e->frame | HD_FRAME_LATENCY, HOOK_MAX_BATCH, HOOK_BLOCK);
	return e->lat[k] ? 0 : -1;                  /* coder missing: the engine fails for good */
}

static int hook_admit(struct hd_cb *cb, int k, int idx, const void *slen)
{
	((struct hook_eng *)cb)->len[k][idx] = (uint32_t)*(const size_t *)slen;
	return 1;                                   /* every block has its slot */
}

static int hook_run(struct hd_cb *cb, int k, int n)
{
	struct hook_eng *e = (struct hook_eng *)cb;
	return hipdeflate_lat_run(e->lat[k], e->len[k], (uint32_t)n);
}

/* (no close: these engines keep their contexts as long as the process lives) */
static const struct hd_cb_client g_hook_client = { .open = hook_open, .admit = hook_admit, .run = hook_run };

#define HOOK_ENG_INIT(lv, fr, ld) { .cb = HD_CB_INIT(&g_hook_client, &hd_cb_deflate_policy, &g_st, HOOK_MAX_BATCH), .level = (lv), .frame = (fr), .loud = (ld) }
#define CODEC_ENGS(lv) { HOOK_ENG_INIT(lv, HD_FRAME_RAW, 0), HOOK_ENG_INIT(lv, HD_FRAME_RAW_FLUSH, 0) }
static struct hook_eng g_hook = HOOK_ENG_INIT(1, HD_FRAME_BGZF, 1);
static struct hook_eng g_codec[10][2] = { CODEC_ENGS(0), CODEC_ENGS(1), CODEC_ENGS(2), CODEC_ENGS(3), CODEC_ENGS(4),
					  CODEC_ENGS(5), CODEC_ENGS(6), CODEC_ENGS(7), CODEC_ENGS(8), CODEC_ENGS(9) };
static pthread_once_t g_env_once = PTHREAD_ONCE_INIT, g_knobs_once = PTHREAD_ONCE_INIT;

__attribute__((destructor)) static void hook_stats_print(void)
{
	if (!g_st.on || !g_st.calls)
		return;
	fprintf(stderr, "hipdeflate hook (%d usable CPUs): %lld calls in %lld batches (%.1f blocks each); us per call: wait for a context %.1f, copy in %.1f, "
		"copy out %.1f, member waits for its batch %.1f; us per batch: leader's window %.1f, others' copies %.1f, device %.1f\n",
		hd_cb_deflate.ncpu, (long long)g_st.calls, (long long)g_st.batches, g_st.batches ? (double)g_st.blocks / g_st.batches : 0.0,
		g_st.ctx_wait / 1e3 / g_st.calls, g_st.copy_in / 1e3 / g_st.calls, g_st.copy_out / 1e3 / g_st.calls,
		g_st.member_wait / 1e3 / (g_st.calls - g_st.batches ? g_st.calls - g_st.batches : 1), g_st.window / 1e3 / (g_st.batches ? g_st.batches : 1),
		g_st.ready / 1e3 / (g_st.batches ? g_st.batches : 1), g_st.run / 1e3 / (g_st.batches ? g_st.batches : 1));
}

/* CPUs this process may really use: the affinity mask, cut by the cgroup's CPU quota (a container on a 128-core host
 * with 16 CPUs' worth of quota reports 128 through sysconf: members would spin where they must sleep) */
static int usable_cpus(void)
{
	int n = 0;
	cpu_set_t set;
	if (sched_getaffinity(0, sizeof(set), &set) == 0)
		n = CPU_COUNT(&set);
	if (n <= 0) {
		const long nc = sysconf(_SC_NPROCESSORS_ONLN);
		n = nc > 0 ? (int)nc : 1;
	}
	FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r");              /* cgroup v2: "<quota> <period>" or "max <period>" */
	if (f) {
		long long q = 0, per = 0;
		if (fscanf(f, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) {
			const int c = (int)((q + per - 1) / per);
			if (c >= 1 && c < n)
				n = c;
		}
		fclose(f);
	} else if ((f = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r"))) {       /* cgroup v1 */
		long long q = -1, per = 100000;
		if (fscanf(f, "%lld", &q) != 1)
			q = -1;
		fclose(f);
		FILE *g = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r");
		if (g) {
			if (fscanf(g, "%lld", &per) != 1)
				per = 100000;
			fclose(g);
		}
		if (q > 0 && per > 0) {
			const int c = (int)((q + per - 1) / per);
			if (c >= 1 && c < n)
				n = c;
		}
	}
	const char *o = getenv("HIPDEFLATE_CPUS");
	if (o && *o && atoi(o) > 0)
		n = atoi(o);
	return n;
}

static void parse_env(void)
{
	/* bgzf_compress.c:53-113: name = prefix, level = trailing decimal digits */
	const char *s = getenv("BGZF_METHOD");
	int g_level = 6;                        /* unset / empty: the reference's default is zlib at level 6 (bgzf_compress.c:54,:102) */
	if (s && *s) {
		size_t l = strlen(s), i = l;
		int level = -1, digit = 1;
		while (i > 0 && s[i - 1] >= '0' && s[i - 1] <= '9') {
			if (level < 0)
				level = 0;
			level += digit * (s[i - 1] - '0');
			digit *= 10;
			i--;
		}
		if (i == 3 && !strncasecmp(s, "hip", 3)) {
			g_level = level >= 0 ? level : 1;
		} else {
			/* a name of the reference's table, or an unknown one (its zlib): its level, our coder */
			static const struct { const char *name; int deflt; } ref[] = {
				{ "zlib", 6 }, { "7zip", 2 }, { "7-zip", 2 }, { "zopfli", 1 }, { "miniz", 1 }, { "slz", 1 }, { "libslz", 1 },
				{ "libdeflate", 6 }, { "zlibng", 6 }, { "igzip", 1 }, { "cryptopp", 6 } };
			int deflt = 6;
			for (size_t k = 0; k < sizeof(ref) / sizeof(ref[0]); k++)
				if (strlen(ref[k].name) == i && !strncasecmp(s, ref[k].name, i))
					deflt = ref[k].deflt;
			g_level = level >= 0 ? level : deflt;
			if (g_level > 9)
				g_level = 9;
			fprintf(stderr, "hipdeflate: BGZF_METHOD=%s: this library holds the hip coder only; coding with hip%d\n", s, g_level);
		}
	}
	g_hook.level = g_level;
}

/* the batcher's knobs: read once, by whichever engine runs first (the hook's method above only when the HOOK is first called:
 * a process may have used the codecs long before it sets BGZF_METHOD) */
static long knob(const char *name, long deflt, long least)       /* the variable's value where it is set, not empty and >= least */
{
	const char *v = getenv(name);
	return v && *v && atol(v) >= least ? atol(v) : deflt;
}

static void parse_knobs(void)
{
	struct hd_cb_deflate_knobs *const g = &hd_cb_deflate;
	g->window_us = knob("HIPDEFLATE_BATCH_US", g->window_us, LONG_MIN);
	g->ncpu = usable_cpus();
	g->linger_us = knob("HIPDEFLATE_LINGER_US", g->linger_us, LONG_MIN);
	const char *hs = getenv("HIPDEFLATE_HOOK_STATS");
	g_st.on = hs && *hs && *hs != '0';
	g->max_inflight = (int)knob("HIPDEFLATE_INFLIGHT", g->max_inflight, 1);
	g->merge_inflight = (int)knob("HIPDEFLATE_MERGE_INFLIGHT", g->merge_inflight, 1);
	if (g->merge_inflight > g->max_inflight)
		g->merge_inflight = g->max_inflight;
	g->merge_callers = (int)knob("HIPDEFLATE_MERGE_CALLERS", g->merge_callers, LONG_MIN);
	g->rejoin_us = knob("HIPDEFLATE_REJOIN_US", g->rejoin_us, LONG_MIN);
	g->spin_us = knob("HIPDEFLATE_SPIN_US", g->spin_us, LONG_MIN);
	g->batch_target = (int)knob("HIPDEFLATE_BATCH_BLOCKS", HOOK_MAX_BATCH, LONG_MIN);
	if (g->batch_target < 1)
		g->batch_target = 1;
	if (g->batch_target > HOOK_MAX_BATCH)
		g->batch_target = HOOK_MAX_BATCH;
}

/* a block the latency slots do not take (longer than 0xff00 bytes: not from htslib): one ordinary call */
static int code_alone(void *dst, size_t *dlen, const void *src, size_t slen)
{
	uint64_t off = 0;
	uint32_t len = (uint32_t)slen, olen = 0;
	int32_t st = 0;
	unsigned char *tmp = (unsigned char *)malloc(65536);
	if (!tmp)
		return -1;
	int rc = hipdeflate_batch_deflate((const uint8_t *)src, &off, &len, 1, g_hook.level, HD_FRAME_BGZF, tmp, 65536, 65536, &olen,
					  NULL, &st);
	int ret = rc ? -1 : (st || olen > *dlen) ? 1 : 0;
	if (ret == 1)
		fprintf(stderr, "hip_deflate %d\n", st ? st : 1);
	if (!ret) {
		memcpy(dst, tmp, olen);
		*dlen = olen;
	}
	free(tmp);
	return ret;
}

static int hook_call(struct hook_eng *e, void *_dst, size_t *_dlen, const void *src, size_t slen)
{
	struct hd_cb_seat s;
	if (hd_cb_join(&e->cb, &slen, &s))
		return -1;                                  /* coder missing */
	memcpy(hipdeflate_lat_input(e->lat[s.k], (uint32_t)s.idx), src, slen);      /* own block, no lock held */
	const int rc = hd_cb_wait(&e->cb, &s);
	int ret;
	uint32_t olen = 0;
	int32_t st = 0;
	const uint8_t *m = hipdeflate_lat_output(e->lat[s.k], (uint32_t)s.idx, &olen, NULL, &st);
	if (rc || !m) {
		ret = -1;                                   /* coder missing */
	} else if (st || olen > *_dlen) {
		if (e->loud)
			fprintf(stderr, "hip_deflate %d\n", st ? st : 1);
		ret = 1;                                    /* codec error, bgzf_compress.c:163-169 */
	} else {
		memcpy(_dst, m, olen);                      /* own member, no lock held */
		*_dlen = olen;
		ret = 0;
	}
	hd_cb_leave(&e->cb, &s);
	return ret;
}

int bgzf_compress(void *_dst, size_t *_dlen, const void *src, size_t slen, int level_unused)
{
	(void)level_unused;
	if (!slen) {
		/* bgzf_compress.c:40-51 */
		if (*_dlen < 28)
			return -1;
		*_dlen = 28;
		memcpy(_dst,
		       "\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff"
		       "\x06\0BC\x02\x00"
		       "\x1b\x00"
		       "\x03\x00"
		       "\x00\x00\x00\x00\x00\x00\x00\x00",
		       28);
		return 0;
	}
	pthread_once(&g_env_once, parse_env);
	pthread_once(&g_knobs_once, parse_knobs);
	if (*_dlen < 26)                            /* bgzf_compress.c:116 */
		return -1;
	if (slen > 0x10000)                         /* a BGZF member cannot hold it */
		return 1;
	if (slen > HOOK_BLOCK || __atomic_load_n(&g_hook.cb.failed, __ATOMIC_RELAXED))
		return g_hook.cb.failed ? -1 : code_alone(_dst, _dlen, src, slen);
	return hook_call(&g_hook, _dst, _dlen, src, slen);
}

/* The per-block codecs' way in (hd_api.hip deflate_one): one block of 1 .. 0xff00 bytes whose room covers the latency form's
 * worst case and the stored form -- then the bytes do not depend on the room, and callers with different rooms can share a
 * launch.  0 ok, 1 codec error, -1 the engine cannot run (the caller takes its own context), -2 not for a batch. */
__attribute__((visibility("hidden"))) int hd_codec_batch(unsigned char *dest, size_t *destLen, const unsigned char *src, size_t slen,
							 int level, int flush)
{
	if (level < 0 || level > 9 || !slen || slen > HOOK_BLOCK)
		return -2;
	pthread_once(&g_knobs_once, parse_knobs);
	return hook_call(&g_codec[level][flush ? 1 : 0], dest, destLen, src, slen);
}
