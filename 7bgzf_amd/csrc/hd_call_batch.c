/*
 * hd_call_batch.c -- the caller-batching engine (hd_call_batch.h) and the two policies that drive it: the compress side's
 * (the LD_PRELOAD hook and hip_deflate / hip_deflate_flush, bgzf_hook.c) and the decompress side's (hip_inflate /
 * hip_inflate_flush, hd_api.hip).
 */
#define _GNU_SOURCE
#include <sched.h>
#include <time.h>
#include <unistd.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include "hd_call_batch.h"

static inline int64_t now_ns(void)
{
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	return (int64_t)ts.tv_sec * 1000000000LL + ts.tv_nsec;
}

#if defined(__x86_64__) || defined(__i386__)
#define cpu_relax() __builtin_ia32_pause()
#else
#define cpu_relax() ((void)0)
#endif
#define LOAD(x) __atomic_load_n(&(x), __ATOMIC_RELAXED)
#define MAX(a, b) ((a) > (b) ? (a) : (b))
/* the statistics: counts, and the time of a call cut into consecutive laps on the caller's own clock (its seat's) */
#define ST_ON (e->stats && e->stats->on)
#define ST_ADD(field, v) do { if (ST_ON) __atomic_add_fetch(&e->stats->field, (v), __ATOMIC_RELAXED); } while (0)
#define ST_LAP(field) do { if (ST_ON) { const int64_t t_ = now_ns(); ST_ADD(field, t_ - s->t); s->t = t_; } } while (0)

/* (lock held) the collecting batch goes out with the callers it has */
static void batch_close(struct hd_cb *e, struct hd_cb_batch *b)
{
	__atomic_store_n(&b->state, 2, __ATOMIC_RELEASE);
	__atomic_add_fetch(&e->running, b->n, __ATOMIC_RELAXED);
	__atomic_add_fetch(&e->inflight, 1, __ATOMIC_RELAXED);
	e->open = -1;
}

int hd_cb_join(struct hd_cb *e, const void *req, struct hd_cb_seat *s)
{
	__atomic_add_fetch(&e->active, 1, __ATOMIC_RELAXED);
	pthread_mutex_lock(&e->mu);
	s->t = ST_ON ? now_ns() : 0;
	struct hd_cb_batch *b = NULL;
	int k = -1, r = e->failed;
	while (!r) {
		if ((k = e->open) >= 0) {
			b = &e->batch[k];
			if (e->cl->admit(e, k, b->n, req))
				break;
			batch_close(e, b);        /* it cannot take this call: closed as it stands (its leader finds it so), a new one is opened */
		}
		for (k = 0; k < HD_CB_CTX && __atomic_load_n(&e->batch[k].state, __ATOMIC_ACQUIRE) != 0; k++)
			;
		if (k == HD_CB_CTX) {
			pthread_cond_wait(&e->cv_free, &e->mu);   /* every context is busy: wait for one to drain */
			continue;
		}
		b = &e->batch[k];
		if (!b->opened && (r = e->cl->open(e, k)) != 0) {
			e->failed = r;
			break;
		}
		b->opened = 1;
		b->n = b->ready = b->taken = b->rc = 0;            /* (nobody looks at a free context) */
		__atomic_store_n(&b->state, 1, __ATOMIC_RELEASE);
		e->open = k;
		(void)e->cl->admit(e, k, 0, req);
		break;
	}
	if (r) {
		pthread_mutex_unlock(&e->mu);
		__atomic_sub_fetch(&e->active, 1, __ATOMIC_RELAXED);
		return r;
	}
	s->k = k;
	s->idx = b->n;
	__atomic_store_n(&b->n, s->idx + 1, __ATOMIC_RELAXED);     /* (written under the lock; the leader's window loop reads it without) */
	if (e->pol->complete(e, s->idx + 1))
		batch_close(e, b);
	pthread_mutex_unlock(&e->mu);
	ST_ADD(calls, 1);
	ST_LAP(ctx_wait);
	return 0;
}

/* Members that have waited long enough sleep ON THE BATCH'S STATE WORD (futex): the leader's one FUTEX_WAKE releases
 * all of them at once.  (The condition variable of rounds 1-2 handed its waiters over one by one through its mutex --
 * microseconds each: with 64 callers on 16 cores, where members must sleep to leave the CPUs to the leaders, a 27-block
 * batch took 376 us instead of 115 and the CPU reference won that case, 6.24 GB/s against 4.27.) */
int hd_cb_wait(struct hd_cb *e, struct hd_cb_seat *s)
{
	struct hd_cb_batch *const b = &e->batch[s->k];
	__atomic_add_fetch(&b->ready, 1, __ATOMIC_RELEASE);      /* the caller's block is in */
	ST_LAP(copy_in);
	if (s->idx == 0) {
		/* the LEADER.  Others join while the window is open; whoever completes the batch (hd_cb_join) closes it, or the
		 * leader does when its policy says the window is over */
		struct hd_cb_window w = { .n = 1 };
		w.t0 = w.t_last = now_ns();
		while (__atomic_load_n(&b->state, __ATOMIC_ACQUIRE) == 1) {
			w.t = now_ns();
			const int cur = LOAD(b->n);
			if (cur != w.n) {
				w.n = cur;
				w.t_last = w.t;
			}
			const int how = e->pol->window(e, &w);
			if (how == HD_CB_OVER)
				break;
			if (how == HD_CB_YIELD)
				sched_yield();
			else
				cpu_relax();
		}
		pthread_mutex_lock(&e->mu);
		if (LOAD(b->state) == 1)
			batch_close(e, b);
		const int n = b->n;
		pthread_mutex_unlock(&e->mu);
		ST_LAP(window);
		while (__atomic_load_n(&b->ready, __ATOMIC_ACQUIRE) < n)     /* the others are still copying in */
			cpu_relax();
		ST_LAP(ready);
		b->rc = e->cl->run(e, s->k, n);
		__atomic_store_n(&e->t_returned, now_ns(), __ATOMIC_RELAXED);
		pthread_mutex_lock(&e->mu);
		__atomic_sub_fetch(&e->running, n, __ATOMIC_RELAXED);
		__atomic_sub_fetch(&e->inflight, 1, __ATOMIC_RELAXED);
		pthread_mutex_unlock(&e->mu);
		/* (an exchange, i.e. a full fence: the load of `sleepers` below must not pass this store -- a member that
		 * has counted itself in and still reads state 2 goes to sleep) */
		(void)__atomic_exchange_n(&b->state, 3, __ATOMIC_SEQ_CST);
		ST_ADD(batches, 1);
		ST_ADD(blocks, n);
		ST_LAP(run);
		if (__atomic_load_n(&b->sleepers, __ATOMIC_SEQ_CST))
			syscall(SYS_futex, &b->state, FUTEX_WAKE_PRIVATE, 0x7fffffff, NULL, NULL, 0);
	} else {
		/* a MEMBER: spin for the batch (all members see it within a cache miss of the leader's store), sleep only when
		 * it takes long */
		const int64_t spin = e->pol->member_spin_ns(e), deadline = spin < 0 ? 0 : now_ns() + spin;
		int spins = 0, seen;
		while ((seen = __atomic_load_n(&b->state, __ATOMIC_ACQUIRE)) != 3) {
			if (spin < 0 || ((++spins & 63) == 0 && now_ns() > deadline)) {
				/* (a full fence again: count in, THEN look) */
				__atomic_add_fetch(&b->sleepers, 1, __ATOMIC_SEQ_CST);
				/* (the state may be 1 or 2 here; a change to either wakes nobody, so sleep only on what is seen and
				 * look again: FUTEX_WAIT returns at once when the word has moved on) */
				if (__atomic_load_n(&b->state, __ATOMIC_SEQ_CST) == seen)
					syscall(SYS_futex, &b->state, FUTEX_WAIT_PRIVATE, seen, NULL, NULL, 0);
				__atomic_sub_fetch(&b->sleepers, 1, __ATOMIC_ACQ_REL);
			} else {
				cpu_relax();
			}
		}
		ST_LAP(member_wait);
	}
	return b->rc;
}

void hd_cb_leave(struct hd_cb *e, struct hd_cb_seat *s)
{
	struct hd_cb_batch *const b = &e->batch[s->k];
	const int n = b->n;                                   /* (read before `taken` moves: the last taker frees the context) */
	ST_LAP(copy_out);
	if (__atomic_add_fetch(&b->taken, 1, __ATOMIC_ACQ_REL) == n) {
		pthread_mutex_lock(&e->mu);
		__atomic_store_n(&b->state, 0, __ATOMIC_RELEASE);   /* drained: the context can collect again */
		pthread_cond_broadcast(&e->cv_free);
		pthread_mutex_unlock(&e->mu);
	}
	__atomic_sub_fetch(&e->active, 1, __ATOMIC_RELAXED);
}

void hd_cb_drain(struct hd_cb *e)
{
	pthread_mutex_lock(&e->mu);
	for (int k = 0; k < HD_CB_CTX; k++)
		if (e->batch[k].opened && __atomic_load_n(&e->batch[k].state, __ATOMIC_ACQUIRE) == 0) {
			e->cl->close(e, k);
			e->batch[k].opened = 0;
		}
	e->failed = 0;
	pthread_mutex_unlock(&e->mu);
}

/* ---- the compress side's policy ------------------------------------------------------------------------------------
 * max_inflight: batches on the device at once.  Two run side by side at nearly the price of one at levels 1-2
 * (hipdeflate_lat_run on 8 blocks, level 2: 152 us alone, 173 us each for two), a third and fourth do not (266, 297 us
 * each -- tools/hook_bench.c HOOK_PAR): while two are out, the collecting batch stays open and grows.
 * Round 5: that is the limit for FULL batches (more callers than a batch holds).  A batch that is merely COMPLETE -- every
 * caller that is not on the device has joined -- waits while another is out (merge_inflight) and then for that batch's
 * callers to come back (rejoin_us): sixteen callers had settled into two groups of eight that took turns, each paying for
 * the other's launch (level 6: two batches of 8 side by side 227-240 us each, one of 16 alone 186: a call 280 -> 215 us)
 * ... while at most merge_callers callers are inside the engine; beyond, batches fill by themselves and two side by side
 * win (64 callers, level 6: 403 us a call against 520 merged; 4 / 8 callers: 233 -> 191 / 224 -> 209 us; 16: 257 -> 250;
 * tools/r05_hook_merge.sh, profiles/r05_hook_merge.txt) */
struct hd_cb_deflate_knobs hd_cb_deflate = { .window_us = 60, .linger_us = 8, .spin_us = 400, .rejoin_us = 30, .max_inflight = 2,
					     .merge_inflight = 1, .merge_callers = 16, .batch_target = 1 << 30, .ncpu = 1 };

/* Everybody who could join has: the callers inside the engine that are not in a batch on the device are all here
 * (callers released together by the previous batch come back within microseconds of each other, and count
 * as inside while they copy their members out).  Or the batch is full, or has reached its target and a slot is free. */
static int deflate_complete(struct hd_cb *e, int n)
{
	const struct hd_cb_deflate_knobs *const g = &hd_cb_deflate;
	const int want = LOAD(e->active) - e->running;
	return n >= e->slots || (n >= g->batch_target && e->inflight < g->max_inflight) ||
	       (n >= want && e->inflight < (want + e->running <= g->merge_callers ? g->merge_inflight : g->max_inflight));
}

/* The leader closes the batch himself when nobody has joined for linger_us although callers are missing (they are busy
 * elsewhere), or when the window is over.  While merge_inflight batches are out the window stays open -- 2 ms at most,
 * should one hang --, and when one has come back its callers get rejoin_us to show up, then the linger counts from join
 * to join.  A window of 0 is none. */
static int deflate_window(struct hd_cb *e, struct hd_cb_window *w)
{
	const struct hd_cb_deflate_knobs *const g = &hd_cb_deflate;
	if (g->window_us <= 0)
		return HD_CB_OVER;
	const int64_t deadline = w->t0 + g->window_us * 1000, hard = w->t0 + 2000000;
	const int active = LOAD(e->active);
	const int full = LOAD(e->inflight) >= (w->n >= g->batch_target || active > g->merge_callers ? g->max_inflight : g->merge_inflight);
	const int64_t tr = LOAD(e->t_returned);
	const int64_t quiet = tr > w->t_last ? tr + g->rejoin_us * 1000 : w->t_last + g->linger_us * 1000;
	const int64_t dl = tr > w->t0 && tr + g->window_us * 1000 > deadline ? tr + g->window_us * 1000 : deadline;
	if ((w->t >= dl || w->t >= quiet) && (!full || w->t >= hard))
		return HD_CB_OVER;
	/* with every device slot taken and more callers than CPUs, the leaders in flight and the HIP runtime's
	 * thread need this CPU more than a spinning window does */
	return full && active + 1 >= g->ncpu ? HD_CB_YIELD : HD_CB_SPIN;
}

/* as many callers as cores, or more: a spinning (or yielding) member only keeps a leader -- or the HIP runtime's
 * own thread, which a leader's hipStreamSynchronize waits for -- off its CPU: those members sleep at once (16
 * callers on 16 CPUs, hip2: 4.51 -> 4.76 GB/s); otherwise a member spins spin_us for its batch first */
static int64_t deflate_member_spin_ns(struct hd_cb *e)
{
	return LOAD(e->active) + 1 >= hd_cb_deflate.ncpu ? -1 : hd_cb_deflate.spin_us * 1000;
}

const struct hd_cb_policy hd_cb_deflate_policy = { deflate_complete, deflate_window, deflate_member_spin_ns };

/* ---- the decompress side's policy ----------------------------------------------------------------------------------
 * "Everybody who is inside has joined" is not enough to close a batch: the reference creates its -@N threads one after the
 * other (applet/7bgzf.c:330-345), tens of microseconds apart, and a batch that closes as soon as everybody INSIDE has joined
 * goes out with the first few of them -- `7bgzf -d -@16` ran 180 launches of 4..8 streams for 1030 blocks, two side by side,
 * where 65 launches of 16 do (profiles/r05_dec_trace.txt).  `peak` remembers how many callers have been inside at once:
 * a batch is complete when it holds max(inside now, that peak) less those on the device; a batch the LINGER time closes
 * short of it takes the peak down a quarter at a time (callers have gone).  A lone caller never waits.
 * A batch is ~1.5 ms on the device whatever it holds (one wavefront per stream, the chip is empty), and the device runs two
 * launches side by side but hardly a third (see max_inflight above): so at most two batches are out, and while they are
 * the collecting batch stays open and grows.  Sixteen callers settle into two groups of eight that alternate; without the
 * cap they drifted apart into batches of one to four that queued behind one another (3.0 ms per call where the kernel
 * takes 1.55).  (A batch closed because it refused a call goes out even past the cap.) */
struct hd_cb_inflate_knobs hd_cb_inflate = { .window_ns = 400000, .linger_ns = 60000, .max_inflight = 2 };

static int inflate_complete(struct hd_cb *e, int n)
{
	int peak = LOAD(e->peak);
	const int active = LOAD(e->active);
	if (active > peak)
		__atomic_store_n(&e->peak, peak = active, __ATOMIC_RELAXED);
	return n >= e->slots || (n >= peak - e->running && e->inflight < hd_cb_inflate.max_inflight);
}

/* complete (every caller that is inside and not on the device has joined), or nobody came for the linger time, or the
 * window is over -- and a launch slot is free (20 ms at most, should a batch hang) */
static int inflate_window(struct hd_cb *e, struct hd_cb_window *w)
{
	const struct hd_cb_inflate_knobs *const g = &hd_cb_inflate;
	const int slot = LOAD(e->inflight) < g->max_inflight;
	const int running = LOAD(e->running), peak = LOAD(e->peak), active = LOAD(e->active);
	const int complete = w->n >= MAX(active, peak) - running;
	const int lingered = w->t >= w->t0 + g->window_ns || w->t - w->t_last >= g->linger_ns;
	if (((complete || lingered) && slot) || w->t >= w->t0 + 20000000) {
		if (!complete && lingered && slot)       /* callers have gone: the peak comes down, a quarter at a time */
			__atomic_store_n(&e->peak, MAX(w->n + running, peak - MAX(1, peak / 4)), __ATOMIC_RELAXED);
		return HD_CB_OVER;
	}
	/* two batches are out for a millisecond yet: leave the CPU to their callers, every 16th poll */
	return !slot && (++w->polls & 15) == 0 ? HD_CB_YIELD : HD_CB_SPIN;
}

/* a batch is about a millisecond of device time: look for a moment (a batch of short streams), then sleep on the word */
static int64_t inflate_member_spin_ns(struct hd_cb *e)
{
	return 20000;
}

const struct hd_cb_policy hd_cb_inflate_policy = { inflate_complete, inflate_window, inflate_member_spin_ns };
