/*
 * hd_call_batch.h -- concurrent one-block callers coalesced into one launch: the protocol, written once.
 *
 * htslib's workers call the hook once per block, the reference's -@N threads call hip_deflate / hip_inflate once per
 * block (applet/7bgzf.c:211, :330-345), and each waits for its answer.  Calls that arrive together share a BATCH: every
 * caller copies its own block in and its own answer out with no lock held, the first caller of a batch (its LEADER)
 * keeps it open for a window, launches and publishes the result, the others (MEMBERS) spin on the batch's state word and
 * then sleep on it.  HD_CB_CTX batches can be collecting / on the device side by side.
 *
 * What a batch owns (pinned memory, a stream, a latency context) belongs to the CLIENT and reaches the engine as a table
 * of functions; when a batch is complete and how long its window stays open is the POLICY, one per direction (below).
 * Nothing here knows about DEFLATE.  Plain C, no HIP: tests/native/hook_stress.c runs all of it under the sanitizers.
 */
#ifndef HD_CALL_BATCH_H
#define HD_CALL_BATCH_H
#include <pthread.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(hidden)

#define HD_CB_CTX 8

struct hd_cb;

/* What a batch owns.  `k` is the batch context, `idx` the caller's slot in its batch, `req` what the caller handed to
 * hd_cb_join() */
struct hd_cb_client {
	int (*open)(struct hd_cb *e, int k);                        /* (lock held) context k's resources, once; 0 or the engine's failure */
	/* (lock held) can the collecting batch take this call?  1: its room is reserved; 0: the batch is closed as it stands
	 * and another is opened.  idx 0 is a batch's first call: it starts the batch's bookkeeping and is never refused */
	int (*admit)(struct hd_cb *e, int k, int idx, const void *req);
	int (*run)(struct hd_cb *e, int k, int n);                  /* (no lock) the leader's launch and wait; the batch's rc */
	void (*close)(struct hd_cb *e, int k);                      /* (lock held) release an idle context's resources: hd_cb_drain() */
};

/* what the leader's window loop has seen; `polls` is the policy's own */
struct hd_cb_window {
	int64_t t0, t_last, t;       /* the window opened / somebody last joined / now (ns) */
	int n, polls;                /* callers in the batch now */
};
enum { HD_CB_OVER, HD_CB_SPIN, HD_CB_YIELD };

struct hd_cb_policy {
	int (*complete)(struct hd_cb *e, int n);                       /* (lock held) the n-th caller has joined: close the batch? */
	int (*window)(struct hd_cb *e, struct hd_cb_window *w);        /* (no lock) HD_CB_OVER, or how the leader waits meanwhile */
	int64_t (*member_spin_ns)(struct hd_cb *e);                    /* a member spins this long before it sleeps; < 0: sleeps at once */
};

/* HIPDEFLATE_HOOK_STATS: where the time of a call goes (ns sums).  Whoever owns the engine prints them */
struct hd_cb_stats {
	int on;
	int64_t calls, batches, blocks, copy_in, window, ready, run, member_wait, copy_out, ctx_wait;
};

struct hd_cb_batch {
	/* state: 0 free, 1 collecting, 2 closed (copies in flight / on the device), 3 done.  Changed under the engine's lock
	 * (0 -> 1 -> 2, 3 -> 0) or by the batch's leader (2 -> 3); read with acquire loads by spinning members, and the word
	 * members sleep on (futex) */
	int state;
	int n;                       /* callers admitted (under the lock while collecting, fixed afterwards) */
	int ready, taken;            /* blocks copied in / answers copied out (atomic counters) */
	int sleepers;                /* members of THIS batch asleep on `state` */
	int rc, opened;
};

struct hd_cb {
	pthread_mutex_t mu;
	pthread_cond_t cv_free;      /* a context became free */
	const struct hd_cb_client *cl;
	const struct hd_cb_policy *pol;
	struct hd_cb_stats *stats;   /* or NULL */
	int slots;                   /* callers a batch holds at most */
	int open;                    /* the batch that is collecting, -1 = none */
	int active;                  /* callers inside the engine right now (atomic) */
	int running;                 /* callers of the batches that are closed and not yet done (written under mu) */
	int inflight;                /* those batches (written under mu) */
	int failed;                  /* what open() answered: the engine is down until hd_cb_drain() */
	int peak;                    /* the inflate policy's memory: how many callers have been inside at once */
	int64_t t_returned;          /* when the last batch came back from the device (atomic; 0 = none yet) */
	struct hd_cb_batch batch[HD_CB_CTX];
};
#define HD_CB_INIT(client, policy, st, nslots) { PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, (client), (policy), (st), (nslots), -1 }

/* One call through the engine is join, wait, leave, with the caller's own copies -- no lock held -- in between:
 *   hd_cb_join()   joins the collecting batch or opens one: 0 and the caller's seat, or the engine's failure (no seat);
 *   ... the caller copies its block into slot `idx` of context `k` ...
 *   hd_cb_wait()   plays leader (window, launch, publish) or member (spin, then sleep): the batch's rc;
 *   ... the caller copies its answer out of that slot ...
 *   hd_cb_leave()  the last to leave frees the context. */
struct hd_cb_seat {
	int k, idx;
	int64_t t;                   /* (statistics) where the caller's current lap began */
};
int hd_cb_join(struct hd_cb *e, const void *req, struct hd_cb_seat *s);
int hd_cb_wait(struct hd_cb *e, struct hd_cb_seat *s);
void hd_cb_leave(struct hd_cb *e, struct hd_cb_seat *s);
/* idle contexts are closed and a failure is forgotten */
void hd_cb_drain(struct hd_cb *e);

/* ---- the two policies and their knobs (the clients read the environment into them before the first call) ---------- */
extern const struct hd_cb_policy hd_cb_deflate_policy, hd_cb_inflate_policy;

extern struct hd_cb_deflate_knobs {
	long window_us;              /* HIPDEFLATE_BATCH_US: a leader never waits longer than this for the batch to fill */
	long linger_us;              /* HIPDEFLATE_LINGER_US: ... nor longer than this after the last caller joined */
	long spin_us;                /* HIPDEFLATE_SPIN_US: a member spins this long for its batch before it sleeps */
	long rejoin_us;              /* HIPDEFLATE_REJOIN_US */
	int max_inflight, merge_inflight, merge_callers;   /* HIPDEFLATE_INFLIGHT, _MERGE_INFLIGHT, _MERGE_CALLERS */
	int batch_target;            /* HIPDEFLATE_BATCH_BLOCKS */
	int ncpu;                    /* CPUs this process may really use (HIPDEFLATE_CPUS) */
} hd_cb_deflate;

extern struct hd_cb_inflate_knobs {
	long window_ns, linger_ns;   /* HIPDEFLATE_INFLATE_WINDOW_US / _LINGER_US */
	int max_inflight;            /* HIPDEFLATE_INFLATE_INFLIGHT */
} hd_cb_inflate;

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
