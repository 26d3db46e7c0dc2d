// hd_api.hip -- the C ABI of libhipdeflate.so (include/hipdeflate.h): context,
// device/pinned pools, kernel launches, and the per-block zlibutil-style codecs.
//
// No CPU codec lives here: when no gfx950 device is usable every entry point
// fails loudly (HD_E_NODEVICE + one line on stderr).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "../../include/hipdeflate.h"
#include "hd_call_batch.h"
#include "hd_deflate_static.hpp"
#include "hd_deflate_dynamic.hpp"
#include "hd_deflate_wg.hpp"
#include "hd_emit_wg.hpp"
#include "hd_inflate.hpp"
#include "hd_inflate_lat.hpp"
#include "hd_inflate_size.hpp"
#include "hd_frame.hpp"
#include "hd_compact.hpp"
#include "hd_index.hpp"
#include "hd_range.hpp"
#include "hd_stream.hpp"
#include "hd_carry.hpp"
#include "hd_blocks.hpp"
#include "hd_seek.hpp"
#include "hd_segment.hpp"
#include "hd_tables.hpp"
#include "hd_scratch.hpp"

namespace {

using hd::CrcTables;

#define HD_CHECK(expr)                                                                         \
	do {                                                                                   \
		hipError_t e_ = (expr);                                                        \
		if (e_ != hipSuccess) {                                                        \
			fprintf(stderr, "hipdeflate: %s failed: %s (%s:%d)\n", #expr,          \
				hipGetErrorString(e_), __FILE__, __LINE__);                    \
			return e_ == hipErrorOutOfMemory ? HD_E_NOMEM : HD_E_NODEVICE;         \
		}                                                                              \
	} while (0)

struct Buf {
	void *p = nullptr;
	size_t cap = 0;
	bool pinned = false;
	int reserve(size_t n)
	{
		if (n <= cap)
			return 0;
		free_current();
		size_t want = n + n / 4 + 4096;
		hipError_t e = pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
		if (e != hipSuccess) {
			p = nullptr;
			cap = 0;
			fprintf(stderr, "hipdeflate: %s of %zu bytes failed: %s\n", pinned ? "hipHostMalloc" : "hipMalloc",
				want, hipGetErrorString(e));
			return HD_E_NOMEM;
		}
		cap = want;
		return 0;
	}
	void free_current()
	{
		if (p)
			(void)(pinned ? hipHostFree(p) : hipFree(p));
		p = nullptr;
		cap = 0;
	}
	void release()
	{
		free_current();
		for (void *q : retired)
			(void)(pinned ? hipHostFree(q) : hipFree(q));
		retired.clear();
	}
	// grow while launches on other streams may still use the old allocation: it is kept until release() instead of
	// being freed behind a device-wide synchronisation (a grow-only buffer retires a handful of allocations at most)
	std::vector<void *> retired;
	int grow_keep_old(size_t n)
	{
		if (n <= cap)
			return 0;
		void *old = p;
		const size_t old_cap = cap;
		p = nullptr;
		cap = 0;
		const int r = reserve(n);
		if (r) {                                   // (nothing changed: the caller may settle for less -- batch_deflate_dev_impl)
			p = old;
			cap = old_cap;
			return r;
		}
		if (old)
			retired.push_back(old);
		return r;
	}
};

// A grow-only device buffer that every launch of the library shares: launches on different streams take turns on it
// (guarded by Ctx::mu_dev)
struct SharedScratch {
	Buf buf;
	hipEvent_t ev = nullptr;         // the last launch that used buf: a launch on ANOTHER stream waits for it
	hipStream_t last = nullptr;
	bool used = false;
	int enter(hipStream_t st)
	{
		if (!ev)
			HD_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
		if (used && last != st)                                     // same stream: already in order
			HD_CHECK(hipStreamWaitEvent(st, ev, 0));
		return 0;
	}
	int leave(hipStream_t st)
	{
		HD_CHECK(hipEventRecord(ev, st));
		last = st;
		used = true;
		return 0;
	}
	void drained(hipStream_t st)             // everything on st has finished: nobody need wait for its event any more
	{
		if (last == st)
			used = false;
	}
	void reset()
	{
		buf.release();
		if (ev)
			(void)hipEventDestroy(ev);
		ev = nullptr;
		last = nullptr;
		used = false;
	}
};

// The last encode launch of the device-pointer API: what a gather asks to learn, on the host, whether an encode kernel of
// the library's own is still running beside it (compact_beside below).  Guarded by Ctx::mu_enc.
struct LastEncode {
	hipEvent_t ev = nullptr;         // recorded right behind the launch; created once, no timing
	hipStream_t stream = nullptr;    // (compared only, never used: the caller may have destroyed it since)
	const void *out = nullptr;       // the slots it writes
	int level = 0;
	uint32_t nblocks = 0;
	bool valid = false;
	void reset()
	{
		if (ev)
			(void)hipEventDestroy(ev);
		ev = nullptr;
		valid = false;
	}
};

struct Ctx {
	bool ready = false;
	int failed = 0;
	int device = -1;
	char desc[256] = "hipdeflate (not initialised)";
	hipStream_t stream = nullptr;
	CrcTables *d_ct = nullptr;
	uint32_t *d_stalls = nullptr;    // blocks the workgroup parse gave up on (hipdeflate_stall_count)
	// host-pointer API pools (guarded by mu)
	std::mutex mu;
	Buf d_in, d_meta, d_slots, d_packed, d_scratch, d_dict;
	Buf h_in{ nullptr, 0, true }, h_meta{ nullptr, 0, true }, h_out{ nullptr, 0, true };
	// device-pointer API scratch (token slabs for the dynamic levels), guarded by mu_dev
	std::mutex mu_dev;
	SharedScratch tok, tiles;        // token slabs and segment slots of a launch / the tile sums of a scan
	SharedScratch frame;             // the payload table of a framed inflate or size pass (hd_frame.hpp)
	SharedScratch dict;              // a dictionary call's staged history and what is made of it once per call (DictScratch below)
	hd::WgBeside beside;             // the workgroup levels' emit kernel beside their parse (hd_deflate_wg.hpp), with tok
	// the last encode launch and the grid of the last gather (hipdeflate_test_compact_grid), behind a mutex of their own:
	// level 1 launches without mu_dev
	std::mutex mu_enc;
	LastEncode enc;
	uint32_t compact_grid = 0;
	void stream_drained(hipStream_t st)
	{
		std::lock_guard<std::mutex> lk(mu_dev);
		tok.drained(st);
		tiles.drained(st);
		frame.drained(st);
		dict.drained(st);
	}
	// member index scratch (hd_index.hpp): the bitmap and tile counts of the blob, the candidate list and its successor
	// tables.  An index call waits for its stream before it returns, so calls take turns by holding mu_index.
	std::mutex mu_index;
	Buf d_index, d_cand;
	// ranged reads (hd_range.hpp), behind mu_index too: the per-member and per-query tables of a call, and the members it decodes
	Buf d_range, d_range_out;
	// one stream from a resident buffer (hd_stream.hpp), behind mu_index too: the tables of a window of chunks, and its slots
	Buf d_stream, d_stream_slots;
	// the block index's merge (hd_blocks.hpp), behind mu_index too: the chain's pieces and the rows they become
	Buf d_blocks;
};

// One context per entry of the device list (hipdeflate_init(devices...)).  An entry is a HIP device ordinal;
// the same ordinal may appear twice (HIPDEFLATE_DEVICES=0,0: two independent contexts on one card -- how the multi-device
// hosts are rehearsed on a one-GPU box).  A thread works on the entry hipdeflate_use_device() chose for it (default: entry
// 0); pipes and latency contexts keep the entry they were opened on.
constexpr int HD_MAX_CTX = 32;
Ctx g_all[HD_MAX_CTX];
int g_want[HD_MAX_CTX];              // the device ordinal asked for per entry (-1: from the environment)
int g_nctx = 0;                      // entries configured (0: not yet -- the first use reads the environment)
thread_local int t_cur = 0;
std::mutex g_init_mu;
inline Ctx &cur() { return g_all[t_cur]; }

} // namespace
int hd_probe_lds_order(void);        // hd_selftest.hip
namespace {
// the per-block codecs' pool of latency contexts (deflate_one below), closed by hipdeflate_shutdown()
constexpr int CODEC_LEVELS = 13;                          // levels 0..12 (the kernels clamp above 9)
constexpr size_t CODEC_POOL_MAX = 64;                     // idle contexts kept per level (~200 KiB pinned each)
std::mutex g_codec_mu;
std::vector<hipdeflate_lat *> g_codec_free[CODEC_LEVELS];
void codec_pool_drain()
{
	std::lock_guard<std::mutex> lk(g_codec_mu);
	for (std::vector<hipdeflate_lat *> &f : g_codec_free) {
		for (hipdeflate_lat *c : f)
			hipdeflate_lat_close(c);
		f.clear();
	}
}

void build_crc_tables(CrcTables *t)
{
	const uint32_t poly = 0xEDB88320u;
	for (uint32_t i = 0; i < 256; i++) {
		uint32_t c = i;
		for (int k = 0; k < 8; k++)
			c = (c >> 1) ^ (poly & (0u - (c & 1u)));
		t->T[0][i] = c;
	}
	for (int k = 1; k < 4; k++)
		for (uint32_t i = 0; i < 256; i++)
			t->T[k][i] = (t->T[k - 1][i] >> 8) ^ t->T[0][t->T[k - 1][i] & 0xff];
	// B[k][v]: state (v << 8k) after 1024 zero bytes; B16: after 16; BL: after 1008
	for (int k = 0; k < 4; k++)
		for (uint32_t i = 0; i < 256; i++) {
			uint32_t s = i << (8 * k);
			for (int z = 0; z < 1024; z++) {
				if (z == 16)
					t->B16[k][i] = s;
				if (z == 1008)
					t->BL[k][i] = s;
				s = t->T[0][s & 0xff] ^ (s >> 8);
			}
			t->B[k][i] = s;
		}
	// T16[j][b]: byte b followed by j zero bytes (slicing-by-16)
	for (uint32_t i = 0; i < 256; i++)
		t->T16[0][i] = t->T[0][i];
	for (int j = 1; j < 16; j++)
		for (uint32_t i = 0; i < 256; i++)
			t->T16[j][i] = (t->T16[j - 1][i] >> 8) ^ t->T[0][t->T16[j - 1][i] & 0xff];
	// SL: static litlen codes (RFC 1951 3.2.6), bit-reversed, length extra bits appended, bit count << 16
	{
		auto rev = [](uint32_t c, int bits) {
			uint32_t r = 0;
			for (int i = 0; i < bits; i++)
				r |= ((c >> i) & 1u) << (bits - 1 - i);
			return r;
		};
		auto litlen = [&](uint32_t sym, uint32_t &code, uint32_t &bits) {
			if (sym < 144) { code = rev(0x30 + sym, 8); bits = 8; }
			else if (sym < 256) { code = rev(0x190 + (sym - 144), 9); bits = 9; }
			else if (sym < 280) { code = rev(sym - 256, 7); bits = 7; }
			else { code = rev(0xC0 + (sym - 280), 8); bits = 8; }
		};
		static const uint16_t lbase[29] = { 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
						    67, 83, 99, 115, 131, 163, 195, 227, 258 };
		static const uint8_t lext[29] = { 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3,
						  4, 4, 4, 4, 5, 5, 5, 5, 0 };
		for (uint32_t i = 0; i < 256; i++) {
			uint32_t c, b;
			litlen(i, c, b);
			t->SL[i] = c | (b << 16);
		}
		for (uint32_t len = 3; len <= 258; len++) {
			uint32_t slot = 28;
			while (lbase[slot] > len)
				slot--;
			uint32_t c, b;
			litlen(257 + slot, c, b);
			t->SL[256 + len - 3] = (c | ((len - lbase[slot]) << b)) | ((b + lext[slot]) << 16);
		}
	}
	// P2[j]: 2^j zero bytes appended (each the square of the one before); SM[s][m-1]: m segments' worth
	{
		auto apply = [](const uint32_t (*Z)[256], uint32_t v) {
			return Z[0][v & 0xff] ^ Z[1][(v >> 8) & 0xff] ^ Z[2][(v >> 16) & 0xff] ^ Z[3][v >> 24];
		};
		for (int k = 0; k < 4; k++)
			for (uint32_t i = 0; i < 256; i++) {
				const uint32_t v = i << (8 * k);
				t->P2[0][k][i] = t->T[0][v & 0xff] ^ (v >> 8);
			}
		for (int j = 1; j < 24; j++)
			for (int k = 0; k < 4; k++)
				for (uint32_t i = 0; i < 256; i++)
					t->P2[j][k][i] = apply(t->P2[j - 1], t->P2[j - 1][k][i]);
		static const uint32_t segs[3] = { HD_LAT_SEG_BYTES(1), HD_LAT_SEG_BYTES(2), HD_SEG_BYTES };
		for (int si = 0; si < 3; si++) {
			for (int k = 0; k < 4; k++)
				for (uint32_t i = 0; i < 256; i++) {
					uint32_t v = i << (8 * k);
					for (int j = 0; j < 24; j++)
						if (segs[si] & (1u << j))
							v = apply(t->P2[j], v);
					t->SM[si][0][k][i] = v;
				}
			for (int m = 1; m < 16; m++)                 // (the one-segment operator is complete by now)
				for (int k = 0; k < 4; k++)
					for (uint32_t i = 0; i < 256; i++)
						t->SM[si][m][k][i] = apply(t->SM[si][0], t->SM[si][m - 1][k][i]);
		}
	}
	// K[q] = x^(128 q): appending 16 q zero bytes to the state 0x80000000 (= x^0)
	uint32_t s = 0x80000000u;
	for (int q = 0; q < 64; q++) {
		t->K[q] = s;
		for (int z = 0; z < 16; z++)
			s = t->T[0][s & 0xff] ^ (s >> 8);
	}
}

// (g_init_mu held) the device list, once: an explicit list, or the environment -- HIPDEFLATE_DEVICES=0,1,... (a list),
// HIPDEFLATE_DEVICE / LOCAL_RANK (one ordinal: a torch.distributed rank owns one card), else device 0
void configure_locked(const int *devices, int n)
{
	if (g_nctx)
		return;
	if (devices && n > 0) {
		for (int i = 0; i < n && i < HD_MAX_CTX; i++)
			g_want[g_nctx++] = devices[i];
		return;
	}
	const char *s = getenv("HIPDEFLATE_DEVICES");
	if (s && *s) {
		while (*s && g_nctx < HD_MAX_CTX) {
			char *end = nullptr;
			const long v = strtol(s, &end, 10);
			if (end == s)
				break;
			g_want[g_nctx++] = (int)(v < 0 ? 0 : v);
			s = *end == ',' ? end + 1 : end;
		}
	}
	if (!g_nctx)
		g_want[g_nctx++] = -1;
}

int ctx_init(Ctx &g, int device)
{
	std::lock_guard<std::mutex> lk(g_init_mu);
	if (g.ready)
		return 0;
	if (g.failed)
		return g.failed;
	// HIPDEFLATE_INIT_TRACE=1: where the start-up goes, one line on stderr (profiles/r05_startup.txt)
	const bool trace = getenv("HIPDEFLATE_INIT_TRACE") != nullptr;
	double ts[8];
	int nts = 0;
	auto stamp = [&]() {
		if (trace && nts < 8) {
			struct timespec t;
			clock_gettime(CLOCK_MONOTONIC, &t);
			ts[nts++] = t.tv_sec * 1e3 + t.tv_nsec / 1e6;
		}
	};
	stamp();
	int ndev = 0;
	hipError_t e = hipGetDeviceCount(&ndev);
	stamp();
	if (e != hipSuccess || ndev == 0) {
		fprintf(stderr, "hipdeflate: no HIP device (%s); there is no CPU fallback\n",
			e == hipSuccess ? "device count 0" : hipGetErrorString(e));
		return g.failed = HD_E_NODEVICE;
	}
	if (device < 0) {
		const char *s = getenv("HIPDEFLATE_DEVICE");
		if (!s || !*s)
			s = getenv("LOCAL_RANK");
		device = s && *s ? atoi(s) % ndev : 0;
	}
	if (device >= ndev)
		device = device % ndev;
	hipDeviceProp_t prop;
	HD_CHECK(hipSetDevice(device));
	HD_CHECK(hipGetDeviceProperties(&prop, device));
	if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
		fprintf(stderr, "hipdeflate: device %d is %s; this library holds gfx950 (MI355X) code only\n", device,
			prop.gcnArchName);
		return g.failed = HD_E_NODEVICE;
	}
	stamp();
	HD_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
	stamp();
	CrcTables *h = (CrcTables *)malloc(sizeof(CrcTables));
	build_crc_tables(h);
	stamp();
	HD_CHECK(hipMalloc((void **)&g.d_ct, sizeof(CrcTables)));
	HD_CHECK(hipMemcpy(g.d_ct, h, sizeof(CrcTables), hipMemcpyHostToDevice));
	free(h);
	HD_CHECK(hipMalloc((void **)&g.d_stalls, 16));
	HD_CHECK(hipMemset(g.d_stalls, 0, 16));
	stamp();
	// Several lanes' ds_write_b16 to one table entry in one instruction: the highest lane's data must stay (the parse
	// kernels and their CPU twin lean on it, hd_deflate_static.hpp fetch()).  Probed once per context: on a device
	// that arbitrates differently the streams would still be valid DEFLATE but not the twin's bytes, and ranks of one
	// job could disagree -- refused rather than run.
	if (const int bad = hd_probe_lds_order()) {
		fprintf(stderr, "hipdeflate: device %d failed the LDS store-order probe (%d); this build's encoders are not "
			"reproducible on it and refuse to run\n", device, bad);
		(void)hipFree(g.d_ct);
		g.d_ct = nullptr;
		(void)hipFree(g.d_stalls);
		g.d_stalls = nullptr;
		(void)hipStreamDestroy(g.stream);
		g.stream = nullptr;
		return g.failed = HD_E_NODEVICE;
	}
	stamp();
	if (trace && nts == 7)
		fprintf(stderr, "hipdeflate init (ms): runtime + device count %.1f, set device + properties %.1f, stream %.1f, CRC tables on the CPU %.1f, "
			"first allocations + copy %.1f, first kernel (code object load + LDS order probe) %.1f; total %.1f\n",
			ts[1] - ts[0], ts[2] - ts[1], ts[3] - ts[2], ts[4] - ts[3], ts[5] - ts[4], ts[6] - ts[5], ts[6] - ts[0]);
	g.device = device;
	snprintf(g.desc, sizeof(g.desc), "hipdeflate 0.2 on device %d: %s (%s), %d CUs, %.0f GiB", device, prop.name,
		 prop.gcnArchName, prop.multiProcessorCount, prop.totalGlobalMem / 1073741824.0);
	g.ready = true;
	return 0;
}

// entry `idx` of the device list, created on first use
inline int ensure_ctx(int idx)
{
	Ctx &g = g_all[idx];
	if (g.ready)
		return 0;
	{
		std::lock_guard<std::mutex> lk(g_init_mu);
		configure_locked(nullptr, 0);
		if (idx >= g_nctx)
			return HD_E_ARG;
	}
	return ctx_init(g, g_want[idx]);
}
// the calling thread's context
inline int ensure() { return ensure_ctx(t_cur); }

// the host-pointer entry points may be called from any thread; the device of
// the calling thread must be the context's
inline int bind_device(const Ctx &g)
{
	HD_CHECK(hipSetDevice(g.device));
	return 0;
}
inline int bind_device() { return bind_device(cur()); }

// the methods of a pipe / latency context run on the entry it was opened on, whatever entry the calling thread has chosen
struct OnCtx {
	int keep;
	explicit OnCtx(int idx) : keep(t_cur) { t_cur = idx; }
	~OnCtx() { t_cur = keep; }
};

// the ordinary coding of a batch at `level`: one wave per block
static int code_batch(const hd::DeflateArgs &a, int level, hipStream_t st)
{
	if (level <= 1) {
		hd::DeflateArgs b = a;
		b.level = level;
		if (a.seg_slots)                    // latency segments: the instantiation with priming compiled in
			hipLaunchKernelGGL((hd::k_deflate_static<HD_L1_WIN_BITS, HD_L1_HASH_BITS, false, 0, true>), dim3(a.nblocks),
					   dim3(64), 0, st, b);
		else
			hipLaunchKernelGGL((hd::k_deflate_static<HD_L1_WIN_BITS, HD_L1_HASH_BITS, false>), dim3(a.nblocks), dim3(64), 0, st, b);
		return 0;
	}
	return hd::launch_deflate_dynamic(a, level, st);
}

int launch_deflate(const hd::DeflateArgs &a, int level, hipStream_t st)
{
	if (a.nblocks == 0)
		return 0;
	int r = a.seg_limit
			? hd::launch_deflate_segmented(a, level, st, [&](const hd::DeflateArgs &x) { return code_batch(x, level, st); })
			: code_batch(a, level, st);
	if (r)
		return r;
	if (a.frame == HD_FRAME_ZLIB)
		hipLaunchKernelGGL(hd::k_adler32_patch, dim3(a.nblocks), dim3(64), 0, st, a.in, a.in_off, a.in_len, a.nblocks,
				   a.out, a.out_stride, a.out_len, a.status);
	HD_CHECK(hipGetLastError());
	return 0;
}

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

// one range of a table, between its pinned and its device copy
template <class Table> hipError_t table_copy(const Table &dst, const Table &src, hd::Span s, hipMemcpyKind kind, hipStream_t st)
{
	return hipMemcpyAsync(dst.ptr(s), src.ptr(s), s.bytes, kind, st);
}

/* ---- the ring of slots both streaming pipes run on ----------------------------- */

struct PipeSlot {
	Buf h_in{ nullptr, 0, true }, h_out{ nullptr, 0, true }, h_meta{ nullptr, 0, true };
	Buf d_in, d_meta, d_slots, d_packed;
	hipStream_t st = nullptr;
	size_t nbytes = 0;
	uint32_t nb = 0;
	int state = 0;               // 0 free, 1 being filled, 2 submitted, 3 result held by the caller
};

// `depth` slots handed round in order: one thread fills and submits, one fetches results (tests/pipe_model.py)
struct SlotRing {
	int ctx = 0;                                 // entry of the device list the pipe lives on
	int depth = 0;
	std::vector<PipeSlot> slots;
	std::mutex mu;
	std::condition_variable cv;
	uint64_t n_in = 0, n_sub = 0, n_out = 0;     // slots handed out / submitted / fetched
	int held = -1;

	// A slot's memory is pinned / allocated when the slot is first handed out (fill): pinning costs ~0.3 ms per MiB, and a
	// stream that ends after one batch -- or a caller that wants its first bytes soon -- should not wait for `depth` batches'
	// worth of it.  Only the streams are made here.
	bool open(int depth_)
	{
		ctx = t_cur;
		depth = depth_;
		slots.resize(depth);
		for (PipeSlot &s : slots)
			if (hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) != hipSuccess)
				return false;
		return true;
	}
	// the slot to fill, once it is free: nullptr for input() twice without submit(), or when alloc (the slot's memory, outside
	// the lock; the caller is the one thread that does input() / submit() on this pipe) fails
	template <class Alloc> PipeSlot *fill(Alloc alloc)
	{
		std::unique_lock<std::mutex> lk(mu);
		PipeSlot &s = slots[n_in % depth];
		if (s.state == 1)
			return nullptr;
		cv.wait(lk, [&] { return s.state == 0; });
		lk.unlock();
		{
			const OnCtx on(ctx);
			if (ensure() || bind_device() || (!s.h_in.p && alloc(s)))
				return nullptr;
		}
		lk.lock();
		s.state = 1;
		return &s;
	}
	PipeSlot *filling()                          // the slot input() handed out (nullptr: none)
	{
		std::lock_guard<std::mutex> lk(mu);
		PipeSlot &s = slots[n_in % depth];
		return s.state == 1 ? &s : nullptr;
	}
	void submitted(PipeSlot &s)
	{
		std::lock_guard<std::mutex> lk(mu);
		s.state = 2;
		n_in++;
		n_sub++;
		cv.notify_all();
	}
	PipeSlot *next_result()                      // the previous result goes back to the pool; nullptr: nothing pending
	{
		std::lock_guard<std::mutex> lk(mu);
		if (held >= 0) {
			slots[held].state = 0;
			held = -1;
			cv.notify_all();
		}
		return n_out == n_sub ? nullptr : &slots[n_out % depth];
	}
	void hold(PipeSlot &s)
	{
		std::lock_guard<std::mutex> lk(mu);
		s.state = 3;
		held = (int)(n_out % depth);
		n_out++;
	}
	void close()
	{
		const OnCtx on(ctx);
		Ctx &g = cur();
		(void)hipSetDevice(g.device);
		(void)hipDeviceSynchronize();
		for (PipeSlot &s : slots) {
			for (Buf *b : { &s.h_in, &s.h_out, &s.h_meta, &s.d_in, &s.d_meta, &s.d_slots, &s.d_packed })
				b->release();
			if (s.st) {
				g.stream_drained(s.st);
				(void)hipStreamDestroy(s.st);
			}
		}
	}
};

} // namespace

extern "C" {

int hipdeflate_init(int device)
{
	{
		// device < 0 = "from the environment": HIPDEFLATE_DEVICES (a list) if set, else HIPDEFLATE_DEVICE / LOCAL_RANK /
		// 0 -- the same list every other entry point would configure lazily (-1 used to pin a list of one
		// and HIPDEFLATE_DEVICES was never read by the hosts that call this first)
		std::lock_guard<std::mutex> lk(g_init_mu);
		if (device < 0)
			configure_locked(nullptr, 0);
		else
			configure_locked(&device, 1);
	}
	return ensure();
}

int hipdeflate_init_devices(const int *devices, int n)
{
	if (!devices || n < 1 || n > HD_MAX_CTX)
		return HD_E_ARG;
	{
		std::lock_guard<std::mutex> lk(g_init_mu);
		if (g_nctx) {                                     // a list is already in force: the same one is fine
			if (g_nctx != n)
				return HD_E_ARG;
			for (int i = 0; i < n; i++)
				if (g_want[i] != devices[i] && !(g_all[i].ready && g_all[i].device == devices[i]))
					return HD_E_ARG;
		}
		configure_locked(devices, n);
	}
	const int keep = t_cur;
	int r = 0;
	for (int i = 0; i < n && !r; i++) {
		t_cur = i;
		r = ensure();
	}
	t_cur = keep;
	return r;
}

int hipdeflate_device_count(void)
{
	std::lock_guard<std::mutex> lk(g_init_mu);
	configure_locked(nullptr, 0);
	return g_nctx;
}

int hipdeflate_use_device(int index)
{
	if (index < 0 || index >= hipdeflate_device_count())
		return HD_E_ARG;
	t_cur = index;
	return ensure();
}

int hipdeflate_available(void) { return ensure(); }

uint64_t hipdeflate_stall_count(void)
{
	uint64_t sum = 0;
	std::lock_guard<std::mutex> lk(g_init_mu);
	for (int i = 0; i < HD_MAX_CTX; i++) {
		Ctx &g = g_all[i];
		if (!g.ready || !g.d_stalls)
			continue;
		uint32_t v = 0;
		if (hipSetDevice(g.device) == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
		    hipMemcpy(&v, g.d_stalls, 4, hipMemcpyDeviceToHost) == hipSuccess)
			sum += v;
	}
	return sum;
}

const char *hipdeflate_version(void) { return cur().desc; }

static void infb_drain();

void hipdeflate_shutdown(void)
{
	codec_pool_drain();                                  // the per-block codecs' contexts (their own locks)
	infb_drain();
	std::lock_guard<std::mutex> lk(g_init_mu);
	for (int i = 0; i < HD_MAX_CTX; i++) {
		Ctx &g = g_all[i];
		g.failed = 0;
		if (!g.ready)
			continue;
		(void)hipSetDevice(g.device);
		(void)hipDeviceSynchronize();                        // launches on callers' streams may still use our scratch
		for (Buf *b : { &g.d_in, &g.d_meta, &g.d_slots, &g.d_packed, &g.d_scratch, &g.d_dict, &g.h_in, &g.h_meta, &g.h_out, &g.d_index,
				&g.d_cand, &g.d_range, &g.d_range_out, &g.d_stream, &g.d_stream_slots, &g.d_blocks })
			b->release();
		(void)hipFree(g.d_ct);
		(void)hipFree(g.d_stalls);
		g.d_stalls = nullptr;
		(void)hipStreamDestroy(g.stream);
		g.tok.reset();
		g.tiles.reset();
		g.frame.reset();
		g.dict.reset();
		g.enc.reset();
		g.beside.release();
		g.d_ct = nullptr;
		g.stream = nullptr;
		g.ready = false;
	}
	g_nctx = 0;                                          // the next use configures again (environment or an explicit list)
}

static uint64_t scratch_need(uint32_t nblocks, uint32_t cap, int level, bool latency)
{
	if (level >= 1 && level < HD_WG_LEVEL && latency && cap > HD_LAT_SEG_BYTES(level))      // (the workgroup levels have no segments in any mode)
		return hd::segmented_scratch_bytes(nblocks, cap, level, HD_LAT_SEG_BYTES(level));
	if (level >= 1 && level < HD_WG_LEVEL && cap > HD_SEG_LIMIT)       // (the workgroup levels take a block of any length whole)
		return hd::segmented_scratch_bytes(nblocks, cap, level);
	return level < 2 ? 0 : hd::dynamic_scratch_bytes(nblocks, cap, level, 0, latency);
}

uint64_t hipdeflate_scratch_bytes(uint32_t nblocks, uint32_t max_block, int level)
{
	return scratch_need(nblocks, max_block, level, false);
}

// the longest payload a block of block_bytes can have at `level`, in any form
static uint64_t bound_payload(uint64_t block_bytes, int level)
{
	// (latency mode included: its segments are the smallest, their worst case the largest)
	const uint32_t lat = HD_LAT_SEG_BYTES(level);
	return (level >= 1 && level < HD_WG_LEVEL && block_bytes > lat) ? HD_SEGN_WORST(block_bytes, lat, 0)
								: block_bytes + 5 * (block_bytes / 65535 + 1) + 5;
}

uint64_t hipdeflate_bound(uint64_t block_bytes, int level)
{
	return (bound_payload(block_bytes, level) + 32 + 15) & ~(uint64_t)15;       // + the longest container (20 + 8 bytes)
}

/* ---- device-pointer API ---------------------------------------------------- */

// The emit kernel BESIDE the parse (hd_deflate_wg.hpp launch_wg) needs its two kernels on the device at the same time.  Where the
// process says that kernels run one at a time -- the runtime's launch-blocking and serialising switches, a profiler collecting
// hardware counters (rocprofv3 --pmc dispatches one kernel at a time and exports these variables to its child) -- the emit kernel
// follows the parse as in round 4: the same bytes, and no resident wavefronts waiting (bounded, ~2 s a block) for a parse that
// cannot start.  HIPDEFLATE_NO_BESIDE=1 says the same by hand.
static uint32_t g_test_beside_keep = hd::BESIDE_KEEP_MAX;     // hipdeflate_test_beside
static bool beside_allowed()
{
	auto on = [](const char *name) {
		const char *v = getenv(name);
		return v && *v && strcmp(v, "0") != 0;
	};
	// (read at every launch -- a launch is >= 512 blocks --, so a test can switch it)
	return !on("HIPDEFLATE_NO_BESIDE") && !on("HIP_LAUNCH_BLOCKING") && !on("AMD_SERIALIZE_KERNEL") && !on("ROCPROF_COUNTER_COLLECTION") &&
	       !getenv("ROCPROF_COUNTERS");
}

// The gather BESIDE an encode kernel.  A stream of batches (bench.py, any caller with two buffer sets) gathers batch k in
// a second stream while the encode kernel of batch k + 1 runs, and what the gather takes from that kernel follows the
// bytes it keeps in flight.  Such a gather has the encode kernel's whole time to spare, so it gets the
// small grid (hd_compact.hpp); nothing on the device waits for anything: the rate is fixed at the launch, by what the
// host knows of the library's own last encode launch.
constexpr uint32_t ENCODE_L1_WAVES_PER_CU = 21;               // six LDS units a wavefront (hd_deflate_static.hpp)
static bool stream_capturing(hipStream_t st)
{
	hipStreamCaptureStatus s = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing(st, &s) != hipSuccess) {
		(void)hipGetLastError();                             // (not this launch's error: the answer is "do not ask further")
		return true;
	}
	return s != hipStreamCaptureStatusNone;
}

// right behind launch_deflate of the device-pointer entry.  A failure here costs the next gathers their small grid only.
static void note_encode(Ctx &g, hipStream_t st, const void *out, int level, uint32_t nblocks)
{
	if (!nblocks || stream_capturing(st))
		return;
	std::lock_guard<std::mutex> lk(g.mu_enc);
	LastEncode &e = g.enc;
	e.valid = false;
	if (!e.ev && hipEventCreateWithFlags(&e.ev, hipEventDisableTiming) != hipSuccess) {
		e.ev = nullptr;
		(void)hipGetLastError();
		return;
	}
	if (hipEventRecord(e.ev, st) != hipSuccess) {
		(void)hipGetLastError();
		return;
	}
	e.stream = st;
	e.out = out;
	e.level = level;
	e.nblocks = nblocks;
	e.valid = true;
}

// HIPDEFLATE_GATHER_GRID=full|beside|auto (default auto), read at every launch like beside_allowed()'s variables
static bool compact_beside(Ctx &g, const void *slots, hipStream_t st)
{
	const char *v = getenv("HIPDEFLATE_GATHER_GRID");
	if (v && !strcmp(v, "full"))
		return false;
	if (v && !strcmp(v, "beside"))
		return true;
	if (stream_capturing(st))
		return false;
	std::lock_guard<std::mutex> lk(g.mu_enc);
	const LastEncode &e = g.enc;
	// another stream's, other slots (a gather that waits for its own producer has nothing beside it, as far as the library
	// can know), a real encode (level 0 is a copy the throttled gather would outlast several times) that fills the device
	// (CUs x 21 level-1 wavefronts at once: a smaller launch is over before the gather has started) ...
	if (!e.valid || e.stream == st || e.out == slots || e.level < 1 ||
	    e.nblocks < (uint64_t)hd::compact_device_cus() * ENCODE_L1_WAVES_PER_CU)
		return false;
	// ... and still queued or running
	const hipError_t q = hipEventQuery(e.ev);
	if (q != hipSuccess)
		(void)hipGetLastError();                             // (the runtime keeps "not ready" as the thread's last error)
	return q == hipErrorNotReady;
}

// The segments of a launch (hd_segment.hpp): a slot that could hold a block longer than the segment limit -- HD_SEG_LIMIT;
// the segment size itself in latency mode -- has such blocks coded in segments, the ordinary coding leaves them alone.
// limit 0: no segments (the workgroup levels take a block of any length whole).
struct SegRule {
	uint32_t bytes, limit;
};
static SegRule seg_rule(int level, bool latency, uint32_t room)
{
	const uint32_t seg = latency ? HD_LAT_SEG_BYTES(level) : HD_SEG_BYTES, lim = latency ? seg : HD_SEG_LIMIT;
	return { seg, (level >= 1 && level < HD_WG_LEVEL && room > lim) ? lim : 0u };
}

// What every encode launch sets the same way (the rest of DeflateArgs: zero).  room: the longest block a slot can hold;
// max_in: the longest block of the batch where the host knows the lengths (0: only the device does)
static hd::DeflateArgs deflate_args(const Ctx &g, const void *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
				    int level, int frame, bool latency, void *out, uint64_t out_stride, uint32_t out_cap,
				    uint32_t *out_len, uint32_t *crc, int32_t *status, uint32_t room, uint32_t max_in)
{
	hd::DeflateArgs a{};
	a.in = (const uint8_t *)in;
	a.in_off = in_off;
	a.in_len = in_len;
	a.nblocks = nblocks;
	a.frame = frame;
	a.level = level;
	a.out = (uint8_t *)out;
	a.out_stride = out_stride;
	a.out_cap = out_cap;
	a.out_len = out_len;
	a.crc = crc;
	a.status = status;
	a.ct = g.d_ct;
	a.stalls = g.d_stalls;
	const SegRule seg = seg_rule(level, latency, room);
	a.seg_bytes = seg.bytes;
	a.seg_limit = seg.limit;
	// the workgroup levels: the parse's records are sized by the longest block where the host knows it, else by the slot
	// (k_parse_wg refuses a block longer than its record)
	a.split_max = (level >= HD_WG_LEVEL && max_in) ? max_in : room;
	// ... and in latency mode the member is written by a workgroup, the same bytes (blocks up to 64 KiB; hd_emit_wg.hpp)
	a.lat = (latency && level >= HD_WG_LEVEL && a.split_max <= hd::EW_BLOCK_MAX) ? 1u : 0u;
	return a;
}

// A dictionary call's library scratch (Ctx::dict): [ the history: the used tail of an encode call's dictionary from byte 0, or the
// last bytes of a decode call's dictionary ENDING at byte HD_WG_WINDOW | the table an encode call's history leaves
// (k_dict_table) | a decode call's words: the dictionary's Adler-32, and the one-row table the Adler kernel reads it by ]
struct DictScratch {
	uint8_t *p;
	static constexpr size_t TABLE = HD_WG_WINDOW, WORDS = TABLE + hd::WG_DICT_TABLE_BYTES, BYTES = WORDS + 64;
	uint8_t *history() const { return p; }
	uint8_t *history_end() const { return p + HD_WG_WINDOW; }
	uint32_t *table() const { return (uint32_t *)(p + TABLE); }
	uint64_t *one_off() const { return (uint64_t *)(p + WORDS); }
	uint32_t *one_len() const { return (uint32_t *)(p + WORDS + 8); }
	uint32_t *adler() const { return (uint32_t *)(p + WORDS + 12); }
};
// the bytes of a dictionary an encode call uses: its last 32 KiB at most, in whole pieces of the parse
static inline uint32_t dict_used_bytes(uint32_t dict_len)
{
	return (dict_len < HD_WG_WINDOW ? dict_len : (uint32_t)HD_WG_WINDOW) & ~(uint32_t)(HD_WG_CUT - 1);
}
static bool g_test_dict_replay = false;                       // hipdeflate_test_dict_replay

static int batch_deflate_dev_impl(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int level,
				  int frame, void *out, uint64_t out_stride, uint32_t out_cap, void *out_len,
				  void *crc32, void *status, void *stream, uint32_t max_in, uint32_t prime_max = 0,
				  const void *dict = nullptr, uint32_t dict_len = 0)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	const bool latency = (frame & HD_FRAME_LATENCY) != 0;
	frame &= ~HD_FRAME_LATENCY;
	if (frame < HD_FRAME_RAW || frame > HD_FRAME_GZIP || (out_stride & 15) || ((uintptr_t)out & 15) || !out_len)
		return HD_E_ARG;
	hipStream_t st = (hipStream_t)stream;
	hd::DeflateArgs a = deflate_args(g, in, (const uint64_t *)in_off, (const uint32_t *)in_len, nblocks, level, frame, latency, out,
					 out_stride, out_cap, (uint32_t *)out_len, (uint32_t *)crc32, (int32_t *)status,
					 hd::split_max_block(out_stride, out_cap), max_in);
	// (the chunks of one stream that carry the window: the workgroup levels' throughput form alone -- DeflateArgs::prime_max)
	a.prime_max = (level >= HD_WG_LEVEL && !a.lat) ? prime_max : 0u;
	const uint64_t need = scratch_need(nblocks, a.split_max, level, latency);
	if (!need) {
		if ((r = launch_deflate(a, level, st)))
			return r;
		note_encode(g, st, out, level, nblocks);
		return 0;
	}
	// token slabs of the dynamic levels, segment slots of large blocks: library-owned, grow-only
	std::lock_guard<std::mutex> lk(g.mu_dev);
	// (a re-allocation must not pull the rug from under launches in flight: the old scratch stays alive)
	bool beside_fits = true;
	if (g.tok.buf.grow_keep_old(need)) {
		// (what the emit kernel BESIDE the parse adds -- a second buffer of records, the flag lines -- is an option, not a need:
		// without it the launch runs in the old order)
		const uint64_t extra = (level >= HD_WG_LEVEL && !a.lat) ? hd::wg_beside_bytes(nblocks, a.split_max) : 0;
		if (!extra || extra >= need || g.tok.buf.grow_keep_old(need - extra))
			return HD_E_NOMEM;
		beside_fits = false;
	}
	a.scratch = (uint8_t *)g.tok.buf.p;
	// a preset dictionary (hipdeflate_batch_deflate_dict_dev): its used tail into aligned scratch and, unless a test asks for the
	// replay everywhere, the table it leaves -- once per call, in front of the parse.  (Its scratch grows before either is entered.)
	const uint32_t dict_used = dict_used_bytes(dict_len);
	const bool with_dict = dict_used && level >= HD_WG_LEVEL && !a.lat;
	if (with_dict && g.dict.buf.grow_keep_old(DictScratch::BYTES))
		return HD_E_NOMEM;
	if ((r = g.tok.enter(st)))
		return r;
	hd::WgDict wd;
	if (with_dict) {
		if ((r = g.dict.enter(st)))
			return r;
		const DictScratch ds{ (uint8_t *)g.dict.buf.p };
		HD_CHECK(hipMemcpyAsync(ds.history(), (const uint8_t *)dict + (dict_len - dict_used), dict_used, hipMemcpyDeviceToDevice, st));
		wd.hist = ds.history();
		wd.used = dict_used;
		if (!g_test_dict_replay) {
			wd.table = ds.table();
			hd::launch_dict_table(a, level, wd, st);
		}
	}
	if (level >= HD_WG_LEVEL && !a.lat && !with_dict && beside_fits && beside_allowed() && g.beside.init() == 0) {
		a.beside = &g.beside;
		// (emit wavefronts a CU keeps: three -- but two beside the four-way parse of BGZF-sized blocks, where the third costs the parse
		// more than it takes off the launch's end: encode_l6 123.8 -> 125.8 GB/s, 1 MiB members the other way, 131.1 -> 128.5;
		// tools/r05_keep_ab.sh)
		const uint32_t keep = (HD_WG_WAYS(level) == 4 && a.split_max <= 65536) ? 2u : 3u;
		a.beside_keep = g_test_beside_keep < keep ? g_test_beside_keep : keep;
	}
	if (with_dict) {
		// (a workgroup level's raw members: launch_deflate's work is the workgroup launch alone)
		if (nblocks) {
			hd::launch_wg(a, level, st, &wd);
			HD_CHECK(hipGetLastError());
		}
		if ((r = g.dict.leave(st)))
			return r;
	} else if ((r = launch_deflate(a, level, st))) {
		return r;
	}
	note_encode(g, st, out, level, nblocks);
	return g.tok.leave(st);
}

int hipdeflate_batch_deflate_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int level,
				 int frame, void *out, uint64_t out_stride, uint32_t out_cap, void *out_len,
				 void *crc32, void *status, void *stream)
{
	return batch_deflate_dev_impl(in, in_off, in_len, nblocks, level, frame, out, out_stride, out_cap, out_len, crc32, status,
				      stream, 0);
}

int hipdeflate_batch_deflate_dict_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int level,
				      const void *dict, uint32_t dict_len, void *out, uint64_t out_stride, uint32_t out_cap,
				      void *out_len, void *crc32, void *status, void *stream)
{
	if (!dict && dict_len) {
		const int r = ensure();
		return r ? r : HD_E_ARG;
	}
	// (levels 0..2, a dictionary below one piece: batch_deflate_dev_impl leaves the dictionary alone -- the plain call's bytes)
	return batch_deflate_dev_impl(in, in_off, in_len, nblocks, level, HD_FRAME_RAW, out, out_stride, out_cap, out_len, crc32, status,
				      stream, 0, 0, dict, dict_len);
}

void hipdeflate_test_dict_replay(int on) { g_test_dict_replay = on != 0; }

// the decode launch over a table (one layout on every side: hd_tables.hpp)
static hd::InflateArgs inflate_args(const Ctx &g, const void *in, const hd::DecTable &t, uint32_t nblocks, void *out, bool want_crc,
				    uint32_t flags)
{
	return { (const uint8_t *)in, t.in_off(), t.in_len(), nblocks, (uint8_t *)out, t.out_off(), t.out_cap(), t.out_len(),
		 want_crc ? t.crc() : nullptr, t.status(), g.d_ct, flags };
}

static int launch_inflate(const hd::InflateArgs &a, hipStream_t st)
{
	hipLaunchKernelGGL(hd::k_inflate, dim3(a.nblocks), dim3(64), 0, st, a);
	HD_CHECK(hipGetLastError());
	return 0;
}

// ... and over the caller's own columns
static int batch_inflate_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, void *out,
			     const void *out_off, const void *out_cap, void *out_len, void *crc32, void *status, void *stream,
			     uint32_t flags)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!out_len)
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	return launch_inflate({ (const uint8_t *)in, (const uint64_t *)in_off, (const uint32_t *)in_len, nblocks, (uint8_t *)out,
				(const uint64_t *)out_off, (const uint32_t *)out_cap, (uint32_t *)out_len, (uint32_t *)crc32,
				(int32_t *)status, g.d_ct, flags },
			      (hipStream_t)stream);
}

int hipdeflate_batch_inflate_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, void *out,
				 const void *out_off, const void *out_cap, void *out_len, void *crc32, void *status,
				 void *stream)
{
	return batch_inflate_dev(in, in_off, in_len, nblocks, out, out_off, out_cap, out_len, crc32, status, stream, 0);
}

int hipdeflate_batch_inflate_flush_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, void *out,
				       const void *out_off, const void *out_cap, void *out_len, void *crc32, void *status,
				       void *stream)
{
	return batch_inflate_dev(in, in_off, in_len, nblocks, out, out_off, out_cap, out_len, crc32, status, stream,
				 hd::INF_FLUSHED);
}

/* ---- zlib / gzip members: header, inflate, trailer (hd_frame.hpp), and the size pass (hd_inflate_size.hpp) ---- */

static inline bool member_frame_ok(int frame) { return frame == HD_FRAME_RAW || frame == HD_FRAME_ZLIB || frame == HD_FRAME_GZIP; }

// the payload table of one call in g.frame (the caller holds g.mu_dev and has entered)
using hd::FrameTable;
static int frame_table(Ctx &g, uint32_t n, hipStream_t st, FrameTable &t)
{
	if (g.frame.buf.grow_keep_old(FrameTable::bytes(n)))
		return HD_E_NOMEM;
	t = FrameTable(g.frame.buf.p, n);
	return g.frame.enter(st);
}

int hipdeflate_batch_inflate_size_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
				      void *out_size, void *in_used, void *status, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!member_frame_ok(frame) || !out_size || !in_used || !status)
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	hipStream_t st = (hipStream_t)stream;
	if (frame == HD_FRAME_RAW) {                                  // no headers: the caller's tables are the payload table
		hipLaunchKernelGGL(hd::k_inflate_size, dim3(nblocks), dim3(64), 0, st,
				   hd::SizeArgs{ (const uint8_t *)in, (const uint64_t *)in_off, (const uint32_t *)in_len, nullptr, nullptr, nblocks,
						 0u, (uint32_t *)out_size, (uint32_t *)in_used, (int32_t *)status });
		HD_CHECK(hipGetLastError());
		return 0;
	}
	std::lock_guard<std::mutex> lk(g.mu_dev);
	FrameTable t;
	if ((r = frame_table(g, nblocks, st, t)))
		return r;
	hipLaunchKernelGGL(hd::k_frame_open, dim3(nblocks), dim3(64), 0, st, (const uint8_t *)in, (const uint64_t *)in_off,
			   (const uint32_t *)in_len, nblocks, frame, t.p_off, t.p_len, t.verdict);
	hipLaunchKernelGGL(hd::k_inflate_size, dim3(nblocks), dim3(64), 0, st,
			   hd::SizeArgs{ (const uint8_t *)in, t.p_off, t.p_len, (const uint64_t *)in_off, t.verdict, nblocks,
					 frame == HD_FRAME_GZIP ? 8u : 4u, (uint32_t *)out_size, (uint32_t *)in_used, (int32_t *)status });
	HD_CHECK(hipGetLastError());
	return g.frame.leave(st);
}

int hipdeflate_batch_inflate_framed_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
					void *out, const void *out_off, const void *out_cap, void *out_len, void *check,
					void *in_used, void *status, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!member_frame_ok(frame) || !out_len || !status)
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	hipStream_t st = (hipStream_t)stream;
	hd::InflateArgs a = { (const uint8_t *)in, (const uint64_t *)in_off, (const uint32_t *)in_len, nblocks, (uint8_t *)out,
			      (const uint64_t *)out_off, (const uint32_t *)out_cap, (uint32_t *)out_len, (uint32_t *)check,
			      (int32_t *)status, g.d_ct, 0 };
	if (frame == HD_FRAME_RAW) {                                  // no header, no trailer: the inflate's answer is the member's
		if (in_used)
			hipLaunchKernelGGL(hd::k_inflate_framed, dim3(nblocks), dim3(64), 0, st, hd::InflateFramedArgs{ a, (uint32_t *)in_used });
		else
			hipLaunchKernelGGL(hd::k_inflate, dim3(nblocks), dim3(64), 0, st, a);
		HD_CHECK(hipGetLastError());
		return 0;
	}
	std::lock_guard<std::mutex> lk(g.mu_dev);
	FrameTable t;
	if ((r = frame_table(g, nblocks, st, t)))
		return r;
	hipLaunchKernelGGL(hd::k_frame_open, dim3(nblocks), dim3(64), 0, st, (const uint8_t *)in, (const uint64_t *)in_off,
			   (const uint32_t *)in_len, nblocks, frame, t.p_off, t.p_len, t.verdict);
	a.in_off = t.p_off;
	a.in_len = t.p_len;
	a.crc = frame == HD_FRAME_GZIP ? t.chk : nullptr;
	hipLaunchKernelGGL(hd::k_inflate_framed, dim3(nblocks), dim3(64), 0, st, hd::InflateFramedArgs{ a, t.used });
	if (frame == HD_FRAME_ZLIB)                                   // (a member whose inflate failed has out_len 0: nothing is read)
		hipLaunchKernelGGL(hd::k_chunk_adler, dim3(nblocks), dim3(64), 0, st, (const uint8_t *)out, (const uint64_t *)out_off,
				   (const uint32_t *)out_len, (const uint32_t *)out_cap, nblocks, t.chk);
	hipLaunchKernelGGL(hd::k_frame_close, dim3((nblocks + 255) / 256), dim3(256), 0, st, (const uint8_t *)in,
			   (const uint64_t *)in_off, (const uint64_t *)t.p_off, (const int32_t *)t.verdict, (const uint32_t *)t.used,
			   (const uint32_t *)t.chk, nblocks, frame, (uint32_t *)out_len, (uint32_t *)check, (uint32_t *)in_used,
			   (int32_t *)status);
	HD_CHECK(hipGetLastError());
	return g.frame.leave(st);
}

int hipdeflate_batch_inflate_dict_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
				      const void *dict, uint32_t dict_len, void *out, const void *out_off, const void *out_cap,
				      void *out_len, void *check, void *in_used, void *status, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if ((frame != HD_FRAME_RAW && frame != HD_FRAME_ZLIB) || !out_len || !status || (!dict && dict_len))
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	// (raw members and no dictionary: the framed call's launch as it is -- no scratch, no turn to take)
	if (frame == HD_FRAME_RAW && dict_len == 0)
		return hipdeflate_batch_inflate_framed_dev(in, in_off, in_len, nblocks, frame, out, out_off, out_cap, out_len, check, in_used,
							   status, stream);
	hipStream_t st = (hipStream_t)stream;
	std::lock_guard<std::mutex> lk(g.mu_dev);
	// the payload table, and behind it one more column: the members that do not name the dictionary
	const size_t table_bytes = (FrameTable::bytes(nblocks) + 15) & ~(size_t)15;
	if (g.frame.buf.grow_keep_old(table_bytes + 4 * (size_t)nblocks) || g.dict.buf.grow_keep_old(DictScratch::BYTES))
		return HD_E_NOMEM;
	const FrameTable t(g.frame.buf.p, nblocks);
	uint32_t *const plain = (uint32_t *)((uint8_t *)g.frame.buf.p + table_bytes);
	const DictScratch ds{ (uint8_t *)g.dict.buf.p };
	if ((r = g.frame.enter(st)) || (r = g.dict.enter(st)))
		return r;
	// the window a member starts with: the dictionary's last 32 KiB at most, ending where the kernel's loads are aligned
	const uint32_t D = dict_len < HD_WG_WINDOW ? dict_len : (uint32_t)HD_WG_WINDOW;
	if (D)
		HD_CHECK(hipMemcpyAsync(ds.history_end() - D, (const uint8_t *)dict + (dict_len - D), D, hipMemcpyDeviceToDevice, st));
	hd::InflateDictArgs a{};
	a.in = (const uint8_t *)in;
	a.in_off = (const uint64_t *)in_off;
	a.in_len = (const uint32_t *)in_len;
	a.nblocks = nblocks;
	a.out = (uint8_t *)out;
	a.out_off = (const uint64_t *)out_off;
	a.out_cap = (const uint32_t *)out_cap;
	a.out_len = (uint32_t *)out_len;
	a.crc = (uint32_t *)check;
	a.status = (int32_t *)status;
	a.ct = g.d_ct;
	a.used = in_used ? (uint32_t *)in_used : t.used;
	a.dict_end = ds.history_end();
	a.dict_len = D;
	a.plain = nullptr;
	if (frame == HD_FRAME_RAW) {                                  // no header, no trailer: the inflate's answer is the member's
		hipLaunchKernelGGL(hd::k_dict_inflate, dim3(nblocks), dim3(64), 0, st, a);
	} else {
		// DICTID is the Adler-32 of the WHOLE dictionary as given: one more chunk for the Adler kernel, read where the caller has it
		if (dict_len) {
			HD_CHECK(hipMemsetAsync(ds.one_off(), 0, 8, st));
			HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)ds.one_len(), (int)dict_len, 1, st));
			hipLaunchKernelGGL(hd::k_chunk_adler, dim3(1), dim3(64), 0, st, (const uint8_t *)dict, (const uint64_t *)ds.one_off(),
					   (const uint32_t *)ds.one_len(), (const uint32_t *)nullptr, 1u, ds.adler());
		}
		hipLaunchKernelGGL(hd::k_dict_open, dim3((nblocks + 255) / 256), dim3(256), 0, st, (const uint8_t *)in, (const uint64_t *)in_off,
				   (const uint32_t *)in_len, nblocks, (const uint32_t *)ds.adler(), dict_len ? 1u : 0u, t.p_off, t.p_len, t.verdict,
				   plain);
		a.in_off = t.p_off;
		a.in_len = t.p_len;
		a.crc = nullptr;
		a.used = t.used;
		a.plain = plain;
		hipLaunchKernelGGL(hd::k_dict_inflate, dim3(nblocks), dim3(64), 0, st, a);
		// (a member whose inflate failed has out_len 0: nothing is read)
		hipLaunchKernelGGL(hd::k_chunk_adler, dim3(nblocks), dim3(64), 0, st, (const uint8_t *)out, (const uint64_t *)out_off,
				   (const uint32_t *)out_len, (const uint32_t *)out_cap, nblocks, t.chk);
		hipLaunchKernelGGL(hd::k_frame_close, dim3((nblocks + 255) / 256), dim3(256), 0, st, (const uint8_t *)in,
				   (const uint64_t *)in_off, (const uint64_t *)t.p_off, (const int32_t *)t.verdict, (const uint32_t *)t.used,
				   (const uint32_t *)t.chk, nblocks, frame, (uint32_t *)out_len, (uint32_t *)check, (uint32_t *)in_used,
				   (int32_t *)status);
	}
	HD_CHECK(hipGetLastError());
	if ((r = g.dict.leave(st)))
		return r;
	return g.frame.leave(st);
}

int hipdeflate_scan_sizes_dev(const void *out_len, uint32_t nblocks, uint64_t base, void *dst_off, void *total,
			      void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (nblocks == 0) {
		if (total)
			HD_CHECK(hipMemsetAsync(total, 0, 8, (hipStream_t)stream));
		return 0;
	}
	const uint32_t ntiles = (nblocks + hd::SCAN_TILE - 1) / hd::SCAN_TILE;
	// the tile buffer is one for the whole library: scans on different streams take turns
	std::lock_guard<std::mutex> lk(g.mu_dev);
	if (g.tiles.buf.grow_keep_old((size_t)ntiles * 8))
		return HD_E_NOMEM;
	uint64_t *tiles = (uint64_t *)g.tiles.buf.p;
	hipStream_t st = (hipStream_t)stream;
	if ((r = g.tiles.enter(st)))
		return r;
	hipLaunchKernelGGL(hd::k_scan_tile_sums, dim3(ntiles), dim3(256), 0, st, (const uint32_t *)out_len, nblocks, tiles);
	hipLaunchKernelGGL(hd::k_scan_tiles, dim3(1), dim3(256), 0, st, tiles, ntiles, base, (uint64_t *)total);
	hipLaunchKernelGGL(hd::k_scan_finish, dim3(ntiles), dim3(256), 0, st, (const uint32_t *)out_len, nblocks, tiles,
			   (uint64_t *)dst_off);
	HD_CHECK(hipGetLastError());
	return g.tiles.leave(st);
}

int hipdeflate_compact_dev(const void *slots, uint64_t stride, const void *out_len, const void *dst_off,
			   uint32_t nblocks, void *dst, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (nblocks == 0)
		return 0;
	if ((stride & 3) || ((uintptr_t)slots & 3))
		return HD_E_ARG;
	hipStream_t st = (hipStream_t)stream;
	const uint32_t grid = hd::launch_compact((const uint8_t *)slots, stride, (const uint32_t *)out_len, (const uint64_t *)dst_off,
						 nblocks, (uint8_t *)dst, st, compact_beside(g, slots, st));
	HD_CHECK(hipGetLastError());
	std::lock_guard<std::mutex> lk(g.mu_enc);
	g.compact_grid = grid;
	return 0;
}

int hipdeflate_compact_span_dev(const void *slots, uint64_t stride, const void *out_len, const void *dst_off,
				uint32_t nblocks, void *span, uint64_t span_base, void *stream)
{
	// k_compact only ever forms dst + dst_off[i] with dst_off[i] >= span_base: the address of "stream byte 0"
	return hipdeflate_compact_dev(slots, stride, out_len, dst_off, nblocks, (uint8_t *)span - span_base, stream);
}

/* ---- device-resident container decode --------------------------------------- */

// exclusive 64-bit prefix sum of len[0..n) into dst (n > 0), plus base, the sum (without base) into *total: the three scan kernels on scratch of the caller
static void index_scan(const uint32_t *len, uint32_t n, uint64_t *tiles, uint64_t *dst, uint64_t *total, hipStream_t st,
		       uint64_t base = 0)
{
	const uint32_t ntiles = (n + hd::SCAN_TILE - 1) / hd::SCAN_TILE;
	hipLaunchKernelGGL(hd::k_scan_tile_sums, dim3(ntiles), dim3(256), 0, st, len, n, tiles);
	hipLaunchKernelGGL(hd::k_scan_tiles, dim3(1), dim3(256), 0, st, tiles, ntiles, base, total);
	hipLaunchKernelGGL(hd::k_scan_finish, dim3(ntiles), dim3(256), 0, st, len, n, tiles, dst);
}
static_assert(hd::SCRATCH_SCAN_TILE == hd::SCAN_TILE, "hd_scratch.hpp counts the tiles index_scan uses");

// what a call with a summary does first: the library is up, the summary is there and zeroed
static int enter_call(void *summary, size_t bytes)
{
	const int r = ensure();
	if (r || !summary)
		return r ? r : HD_E_ARG;
	memset(summary, 0, bytes);
	return 0;
}

/* The chain index, which the member index and the stream indexes share: the sorted candidate list (chain_candidates), the
   caller's links between candidates, the true chain out of the links and every link's rank on it (chain_rank), the caller's
   rows and verdict, the summary read back (chain_read).  Scratch: hd::IndexBitmap in d_index (w: its words), hd::IndexCand in
   d_cand (c). */

// Pass 1 and 2 over src[0, n).  lo == nullptr: the member index's (k_index_flag, k_index_write); no candidate leaves d_cand
// alone.  Else a stream index's: the markers from *lo on (k_stream_flag, k_stream_write) behind candidate 0, *lo itself.
// any_lo (INDEX_ANY, lo == nullptr): the member index's passes with the matcher of members that state no length, from *any_lo on.
static int chain_candidates(Ctx &g, const uint8_t *src, uint64_t n, const uint32_t *lo, hd::IndexKind kind, uint32_t max_members,
			    hd::IndexWords *&w, hd::IndexCand &c, uint32_t &ncand, hipStream_t st, const uint64_t *any_lo = nullptr)
{
	const uint64_t nwords = (n + hd::IDX_WORD - 1) / hd::IDX_WORD, ntb64 = (nwords + hd::IDX_TILE_WORDS - 1) / hd::IDX_TILE_WORDS;
	if (ntb64 > 0x7fffffffu)
		return HD_E_ARG;
	const uint32_t ntb = (uint32_t)ntb64;
	if (g.d_index.reserve(hd::IndexBitmap::bytes(ntb, nwords, lo != nullptr)))
		return HD_E_NOMEM;
	const hd::IndexBitmap b(g.d_index.p, ntb, nwords, lo != nullptr);
	w = b.w;
	uint64_t found = 0;
	HD_CHECK(hipMemsetAsync(b.w, 0, sizeof *b.w, st));
	if (ntb) {
		if (lo)
			hipLaunchKernelGGL(hd::k_stream_flag, dim3(ntb), dim3(256), 0, st, src, n, (uint64_t)*lo, b.bitmap, b.tile_cnt);
		else if (any_lo)
			hipLaunchKernelGGL(hd::k_any_flag, dim3(ntb), dim3(256), 0, st, src, n, *any_lo, b.bitmap, b.tile_cnt);
		else
			hipLaunchKernelGGL(hd::k_index_flag, dim3(ntb), dim3(256), 0, st, src, n, b.bitmap, b.tile_cnt);
		index_scan(b.tile_cnt, ntb, b.tiles, b.tile_off, &b.w->ncand, st);
		HD_CHECK(hipGetLastError());
		HD_CHECK(hipMemcpyAsync(&found, &b.w->ncand, 8, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
	}
	if (found + (lo ? 1 : 0) > 0x7fffffffu)                                  // candidate indices, and ncand + 255, stay well inside 32 bits
		return HD_E_NOMEM;
	ncand = (uint32_t)found + (lo ? 1 : 0);
	if (ncand == 0)
		return 0;
	const size_t max_rows = lo ? ncand : max_members;
	if (g.d_cand.reserve(hd::IndexCand::bytes(ncand, max_rows, kind)))
		return HD_E_NOMEM;
	c = hd::IndexCand(g.d_cand.p, ncand, max_rows, kind);
	if (!lo) {
		if (any_lo)
			hipLaunchKernelGGL(hd::k_any_write, dim3(ntb), dim3(256), 0, st, src, n, *any_lo, (const uint64_t *)b.bitmap, nwords,
					   (const uint64_t *)b.tile_off, c.pos);
		else
			hipLaunchKernelGGL(hd::k_index_write, dim3(ntb), dim3(256), 0, st, src, n, (const uint64_t *)b.bitmap, nwords,
					   (const uint64_t *)b.tile_off, c.pos);
		return 0;
	}
	HD_CHECK(hipMemsetAsync(c.pos, 0, 8, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)c.pos, (int)*lo, 1, st));
	if (ncand > 1)
		hipLaunchKernelGGL(hd::k_stream_write, dim3(ntb), dim3(256), 0, st, src, n, (uint64_t)*lo, (const uint64_t *)b.bitmap, nwords,
				   (const uint64_t *)b.tile_off, c.pos + 1);
	return 0;
}

// The true chain from the links in succ0 and mark: rounds until 2^rounds >= ncand (a chain has at most ncand rows), jump
// the column k_index_jump reads; then every marked candidate's rank, over the successor tables, which are dead by then.
// *nrows: the chain's length.
static int chain_rank(const hd::IndexCand &c, uint32_t ncand, const uint32_t *jump, hd::IndexWords *w, uint64_t *nrows, hipStream_t st)
{
	uint32_t *succ0 = c.succ0, *succ1 = c.succ1;
	for (uint64_t reach = 1; reach < ncand; reach *= 2) {
		hipLaunchKernelGGL(hd::k_index_jump, dim3((ncand + 255) / 256), dim3(256), 0, st, (const uint32_t *)succ0, succ1, jump, c.mark, ncand);
		std::swap(succ0, succ1);
	}
	index_scan(c.mark, ncand, c.tiles, c.rank, &w->rows, st);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(nrows, &w->rows, 8, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	return 0;
}

// behind the caller's verdict kernel: the four words it leaves, into the four fields either summary has for them
static int chain_read(const hd::IndexWords *w, uint64_t *rows, uint64_t *out_bytes, uint64_t *end_offset, uint32_t *status, hipStream_t st)
{
	hd::IndexWords h;
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&h, w, offsetof(hd::IndexWords, ncand), hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	*rows = h.rows, *out_bytes = h.out_bytes, *end_offset = h.end_offset, *status = (uint32_t)h.status;
	return 0;
}

int hipdeflate_index_members_dev(const void *blob, uint64_t nbytes, uint32_t max_members, void *in_off, void *in_len,
				 void *out_size, void *out_off, void *crc_want, hipdeflate_member_summary *summary, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!summary || ((uintptr_t)blob & 15) || (nbytes && !blob))
		return HD_E_ARG;
	memset(summary, 0, sizeof *summary);
	if (nbytes == 0)
		return 0;
	hipStream_t st = (hipStream_t)stream;
	const uint8_t *src = (const uint8_t *)blob;
	std::lock_guard<std::mutex> lk(g.mu_index);
	hd::IndexWords *w = nullptr;
	hd::IndexCand c;
	uint32_t ncand = 0;
	if ((r = chain_candidates(g, src, nbytes, nullptr, hd::INDEX_MEMBERS, max_members, w, c, ncand, st)))
		return r;
	const uint32_t nwg = (ncand + 255) / 256;
	uint64_t nrows = 0;
	if (ncand) {
		hipLaunchKernelGGL(hd::k_index_links, dim3(nwg), dim3(256), 0, st, src, nbytes, (const uint64_t *)c.pos, ncand, c.succ0,
				   c.hdr, c.total, c.mark);
		if ((r = chain_rank(c, ncand, c.total, w, &nrows, st)))
			return r;
		if (nrows) {
			const uint32_t ntab = (uint32_t)(nrows < max_members ? nrows : max_members);
			hipLaunchKernelGGL(hd::k_members_tables, dim3(nwg), dim3(256), 0, st, src, (const uint64_t *)c.pos, (const uint32_t *)c.hdr,
					   (const uint32_t *)c.total, (const uint32_t *)c.mark, (const uint64_t *)c.rank, ncand, nrows, max_members,
					   (uint64_t *)in_off, (uint32_t *)in_len, (uint32_t *)out_size, (uint32_t *)crc_want, &w->end_offset);
			if (ntab)
				index_scan((const uint32_t *)out_size, ntab, c.tiles, (uint64_t *)out_off, &w->out_bytes, st);
		}
	}
	hipLaunchKernelGGL(hd::k_index_verdict, dim3(1), dim3(1), 0, st, src, nbytes, nrows, max_members, &w->rows);
	return chain_read(w, &summary->nmembers, &summary->out_bytes, &summary->end_offset, &summary->status, st);
}

// hipdeflate_index_members_any_dev under mu_index: the chain index with a links pass in two steps around the sizing of the
// candidates that state no length (hd_index.hpp).  The passes run over blob from the 16-byte granule of first_offset on,
// and the candidates' positions count from there.
static int members_any_index(Ctx &g, const uint8_t *blob, uint64_t nbytes, uint64_t first_offset, uint32_t max_members, uint32_t max_in,
			     void *in_off, void *in_len, void *out_size, void *out_off, void *crc_want,
			     hipdeflate_member_any_summary *summary, hipStream_t st)
{
	const uint64_t base = first_offset & ~(uint64_t)15, lo = first_offset - base, n = nbytes - base;
	const uint8_t *src = blob + base;
	hd::IndexWords *w = nullptr;
	hd::IndexCand c;
	uint32_t ncand = 0;
	int r;
	if ((r = chain_candidates(g, src, n, nullptr, hd::INDEX_ANY, max_members, w, c, ncand, st, &lo)))
		return r;
	const uint32_t nwg = (ncand + 255) / 256;
	uint64_t nrows = 0, nsized = 0;
	if (ncand) {
		hipLaunchKernelGGL(hd::k_any_classify, dim3(nwg), dim3(256), 0, st, src, n, (const uint64_t *)c.pos, ncand, c.cls, c.hdr, c.total,
				   c.asize, c.tosize);
		index_scan(c.tosize, ncand, c.tiles, c.rank, &w->spare, st);
		HD_CHECK(hipGetLastError());
		HD_CHECK(hipMemcpyAsync(&nsized, &w->spare, 8, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
		if (nsized) {
			const uint32_t ns = (uint32_t)nsized;
			hipLaunchKernelGGL(hd::k_any_compact, dim3(nwg), dim3(256), 0, st, (const uint32_t *)c.tosize, (const uint64_t *)c.rank, ncand,
					   c.sub);
			hipLaunchKernelGGL(hd::k_member_open, dim3(ns), dim3(64), 0, st, src, n, (const uint64_t *)c.pos, (const uint32_t *)c.sub, ns,
					   max_in, c.hdr, c.astat);
			hipLaunchKernelGGL(hd::k_inflate_member, dim3(ns), dim3(64), 0, st,
					   hd::MemberArgs{ src, c.pos, c.sub, ns, max_in, n, c.hdr, c.asize, c.total, c.astat });
		}
		hipLaunchKernelGGL(hd::k_any_links, dim3(nwg), dim3(256), 0, st, n, lo, max_in, (const uint64_t *)c.pos, ncand,
				   (const uint32_t *)c.tosize, (const int32_t *)c.astat, c.cls, (const uint32_t *)c.total, c.succ0, c.mark);
		if ((r = chain_rank(c, ncand, c.total, w, &nrows, st)))
			return r;
		if (nrows) {
			const uint32_t ntab = (uint32_t)(nrows < max_members ? nrows : max_members);
			hipLaunchKernelGGL(hd::k_any_tables, dim3(nwg), dim3(256), 0, st, src, base, (const uint64_t *)c.pos, (const uint32_t *)c.hdr,
					   (const uint32_t *)c.total, (const uint32_t *)c.asize, (const uint32_t *)c.tosize, (const uint32_t *)c.mark,
					   (const uint64_t *)c.rank, ncand, nrows, max_members, (uint64_t *)in_off, (uint32_t *)in_len,
					   (uint32_t *)out_size, (uint32_t *)crc_want, &w->end_offset);
			if (ntab)
				index_scan((const uint32_t *)out_size, ntab, c.tiles, (uint64_t *)out_off, &w->out_bytes, st);
		}
	}
	hipLaunchKernelGGL(hd::k_any_verdict, dim3(1), dim3(1), 0, st, src, n, base, lo, (const uint64_t *)c.pos, (const uint32_t *)c.cls, ncand,
			   nrows, max_members, &w->rows);
	summary->ncandidates = ncand;
	summary->nsized = nsized;
	return chain_read(w, &summary->nmembers, &summary->out_bytes, &summary->end_offset, &summary->status, st);
}

int hipdeflate_index_members_any_dev(const void *blob, uint64_t nbytes, uint64_t first_offset, uint32_t max_members, uint32_t max_member_in,
				     void *in_off, void *in_len, void *out_size, void *out_off, void *crc_want,
				     hipdeflate_member_any_summary *summary, void *stream)
{
	Ctx &g = cur();
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	if (((uintptr_t)blob & 15) || (nbytes && !blob) || first_offset > nbytes || max_member_in >= HD_INFLATE_MAX_IN ||
	    (max_members && (!in_off || !in_len || !out_size || !out_off || !crc_want)))
		return HD_E_ARG;
	summary->end_offset = first_offset;
	if (first_offset == nbytes)
		return 0;
	std::lock_guard<std::mutex> lk(g.mu_index);
	return members_any_index(g, (const uint8_t *)blob, nbytes, first_offset, max_members,
				 max_member_in ? max_member_in : (uint32_t)HD_INFLATE_MAX_IN - 1, in_off, in_len, out_size, out_off, crc_want, summary,
				 (hipStream_t)stream);
}

int hipdeflate_verify_members_dev(const void *status, const void *out_len, const void *crc32, const void *out_size,
				  const void *crc_want, uint32_t nmembers, uint64_t *first_bad, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!first_bad)
		return HD_E_ARG;
	*first_bad = nmembers;
	if (nmembers == 0)
		return 0;
	if (!status || !out_len || !crc32 || !out_size || !crc_want)
		return HD_E_ARG;
	hipStream_t st = (hipStream_t)stream;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_index.reserve(hd::IndexBitmap::bytes()))
		return HD_E_NOMEM;
	uint32_t *d_bad = &hd::IndexBitmap(g.d_index.p).w->first, bad = hd::IDX_NIL;
	HD_CHECK(hipMemsetAsync(d_bad, 0xff, 4, st));
	hipLaunchKernelGGL(hd::k_members_verify, dim3((nmembers + 255) / 256), dim3(256), 0, st, (const int32_t *)status,
			   (const uint32_t *)out_len, (const uint32_t *)crc32, (const uint32_t *)out_size, (const uint32_t *)crc_want,
			   nmembers, d_bad);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (bad != hd::IDX_NIL)
		*first_bad = bad;
	return 0;
}

// The queries of a ranged read on a table of n rows -- a container's members, or one stream's rows (hd_seek.hpp): lengths,
// first rows and coverage; coverage -> selection, ranks, the layout in the scratch.  *h: the words read back, of which the
// summary gets its four counts.  (Synchronises the stream.)
static int range_plan(const hd::RangeTables &t, const void *in_off, const void *in_len, const void *out_size, const void *out_off, uint32_t n,
		      int kind, const void *q_begin, const void *q_end, uint32_t nqueries, void *dst_off, void *q_len, void *q_status,
		      hd::RangeWords *h, hipdeflate_range_summary *summary, hipStream_t st)
{
	const uint32_t wg_n = (n + 255) / 256, wg_q = (nqueries + 255) / 256;
	hd::RangeWords *w = t.w;
	HD_CHECK(hipMemsetAsync(w, 0, offsetof(hd::RangeWords, bad_row), st));
	HD_CHECK(hipMemsetAsync(&w->bad_row, 0xff, 4, st));
	HD_CHECK(hipMemsetAsync(t.cover, 0, ((size_t)n + 1) * 4, st));
	hipLaunchKernelGGL(hd::k_range_resolve, dim3(wg_q), dim3(256), 0, st, (const uint64_t *)in_off, (const uint32_t *)in_len,
			   (const uint32_t *)out_size, (const uint64_t *)out_off, n, kind, (const uint64_t *)q_begin,
			   (const uint64_t *)q_end, nqueries, (uint32_t *)q_len, (int32_t *)q_status, t.q_pieces, t.q_first, t.q_from, t.cover,
			   &w->nrefused);
	index_scan((const uint32_t *)q_len, nqueries, t.tiles, (uint64_t *)dst_off, &w->out_bytes, st);
	index_scan(t.q_pieces, nqueries, t.tiles, t.piece_off, &w->pieces, st);
	index_scan(t.cover, n + 1, t.tiles, t.cover_scan, &w->cover_total, st);
	hipLaunchKernelGGL(hd::k_range_select, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)t.cover_scan, (const uint32_t *)out_size, n,
			   t.sel, t.sel_size);
	index_scan(t.sel, n, t.tiles, t.rank, &w->nselected, st);
	index_scan(t.sel_size, n, t.tiles, t.scratch_off, &w->sel_bytes, st);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(h, w, sizeof *h, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	summary->out_bytes = h->out_bytes;
	summary->nselected = h->nselected;
	summary->sel_bytes = h->sel_bytes;
	summary->nrefused = h->nrefused;
	return 0;
}

int hipdeflate_read_ranges_dev(const void *blob, const void *in_off, const void *in_len, const void *out_size, const void *out_off,
			       const void *crc_want, uint32_t nmembers, int kind, const void *q_begin, const void *q_end,
			       uint32_t nqueries, void *dst, uint64_t dst_cap, void *dst_off, void *q_len, void *q_status,
			       hipdeflate_range_summary *summary, void *stream)
{
	Ctx &g = cur();
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	summary->bad_member = nmembers;
	if (((uintptr_t)blob & 15) || (kind != HD_RANGE_BYTES && kind != HD_RANGE_VOFFSET) || (!dst && dst_cap) ||
	    nmembers > 0x7fffffffu || nqueries > 0x7fffffffu ||                       // (n + 1 and n + 255 stay inside 32 bits)
	    (nmembers && (!blob || !in_off || !in_len || !out_size || !out_off || !crc_want)) ||
	    (nqueries && (!q_begin || !q_end || !dst_off || !q_len || !q_status)))
		return HD_E_ARG;
	if (nmembers == 0 || nqueries == 0)
		return 0;
	hipStream_t st = (hipStream_t)stream;
	const size_t n = nmembers, nq = nqueries;
	const uint32_t wg_n = (nmembers + 255) / 256;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_range.reserve(hd::RangeTables::bytes(n, nq)))
		return HD_E_NOMEM;
	const hd::RangeTables t(g.d_range.p, n, nq);
	hd::RangeWords *w = t.w, h;
	if ((r = range_plan(t, in_off, in_len, out_size, out_off, nmembers, kind, q_begin, q_end, nqueries, dst_off, q_len, q_status, &h, summary, st)))
		return r;
	if (h.out_bytes > dst_cap) {
		summary->status = 3;
		return 0;
	}
	if (h.nselected == 0)                                                    // no query took a byte
		return 0;
	// the selected members, inflated back to back into the scratch and held to their trailers
	const uint32_t nsel = (uint32_t)h.nselected;
	if (g.d_range_out.reserve(h.sel_bytes + 16))
		return HD_E_NOMEM;
	uint8_t *scratch = (uint8_t *)g.d_range_out.p;
	hipLaunchKernelGGL(hd::k_range_tables, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)in_off, (const uint32_t *)in_len,
			   (const uint32_t *)out_size, (const uint32_t *)crc_want, (const uint32_t *)t.sel, (const uint64_t *)t.rank,
			   (const uint64_t *)t.scratch_off, nmembers, t.c_in_off, t.c_in_len, t.c_out_off, t.c_out_cap, t.c_crc_want, t.c_member);
	if ((r = batch_inflate_dev(blob, t.c_in_off, t.c_in_len, nsel, scratch, t.c_out_off, t.c_out_cap, t.c_out_len, t.c_crc, t.c_status,
				   stream, 0)))
		return r;
	hipLaunchKernelGGL(hd::k_members_verify, dim3((nsel + 255) / 256), dim3(256), 0, st, (const int32_t *)t.c_status,
			   (const uint32_t *)t.c_out_len, (const uint32_t *)t.c_crc, (const uint32_t *)t.c_out_cap,
			   (const uint32_t *)t.c_crc_want, nsel, &w->bad_row);
	hipLaunchKernelGGL(hd::k_range_verdict, dim3(1), dim3(1), 0, st, (const uint32_t *)&w->bad_row, (const uint32_t *)t.c_member,
			   nmembers, &w->bad_member);
	// every query's run of the scratch -> dst + dst_off[q], in pieces over a persistent grid
	const uint64_t grid_cap = (uint64_t)hd::compact_device_cus() * hd::COMPACT_WAVES_PER_CU;
	hipLaunchKernelGGL(hd::k_range_gather, dim3((uint32_t)(h.pieces < grid_cap ? h.pieces : grid_cap)), dim3(64), 0, st,
			   (const uint8_t *)scratch, (const uint64_t *)t.scratch_off, (const uint64_t *)out_off, (const uint32_t *)t.q_first,
			   (const uint64_t *)t.q_from, (const uint32_t *)q_len, (const uint64_t *)dst_off, (const uint64_t *)t.piece_off,
			   nqueries, h.pieces, (uint8_t *)dst);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&h.bad_member, &w->bad_member, 8, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	summary->bad_member = h.bad_member;
	if (h.bad_member != nmembers)
		summary->status = 2;
	return 0;
}

/* ---- one stream from a resident buffer (hd_stream.hpp) ------------------------ */

static uint32_t g_test_stream_window = 0;                     // hipdeflate_test_stream_window
static inline uint32_t stream_hdr(int frame) { return frame == HD_FRAME_GZIP ? 10u : frame == HD_FRAME_ZLIB ? 2u : 0u; }
static inline uint32_t stream_trl(int frame) { return frame == HD_FRAME_GZIP ? 8u : frame == HD_FRAME_ZLIB ? 4u : 0u; }
static inline bool stream_frame_ok(int frame) { return frame == HD_FRAME_RAW || frame == HD_FRAME_ZLIB || frame == HD_FRAME_GZIP; }
static inline bool stream_chunk_ok(uint32_t c) { return c >= 16 && c <= (64u << 20) && !(c & 15); }
constexpr uint32_t STREAM_MAX_PARTS = 0x7fffffffu;            // (n + 1, n + 255 and n + SCAN_TILE stay inside 32 bits)

uint64_t hipdeflate_stream_bound(uint64_t nbytes, uint32_t chunk_bytes, int level, int frame)
{
	if (!stream_chunk_ok(chunk_bytes))
		return 0;
	const uint64_t full = nbytes / chunk_bytes, rest = nbytes % chunk_bytes;
	return stream_hdr(frame) + full * bound_payload(chunk_bytes, level) + (rest ? bound_payload(rest, level) : 0) + 2 +
	       stream_trl(frame);
}

void hipdeflate_test_stream_window(uint32_t chunks) { g_test_stream_window = chunks; }

// check[] / len[] of n parts folded onto *carry.  sum: u64[3] { the parts' bytes, two accumulators }; tiles: the scan's;
// prefix: u64[n]
static int fold_launch(const uint32_t *check, const uint32_t *len, uint32_t n, uint32_t kind, uint64_t *tiles, uint64_t *prefix,
		       uint64_t *sum, uint32_t *carry, hipStream_t st)
{
	HD_CHECK(hipMemsetAsync(sum, 0, 24, st));
	if (n) {
		index_scan(len, n, tiles, prefix, sum, st);
		const uint32_t wgs = (n + 255) / 256;
		hipLaunchKernelGGL(hd::k_check_combine, dim3(wgs < hd::FOLD_GRID ? wgs : hd::FOLD_GRID), dim3(256), 0, st, check, len,
				   (const uint64_t *)prefix, (const uint64_t *)sum, n, kind, sum + 1);
	}
	hipLaunchKernelGGL(hd::k_check_combine_finish, dim3(1), dim3(64), 0, st, (const uint64_t *)(sum + 1),
			   n ? (const uint64_t *)sum : (const uint64_t *)nullptr, kind, carry);
	HD_CHECK(hipGetLastError());
	return 0;
}

int hipdeflate_check_combine_dev(const void *check, const void *len, uint32_t n, int kind, uint32_t *result, void *stream)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!result || (kind != (int)hd::CHECK_CRC32 && kind != (int)hd::CHECK_ADLER32) || n > STREAM_MAX_PARTS || (n && (!check || !len)))
		return HD_E_ARG;
	hipStream_t st = (hipStream_t)stream;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_stream.reserve(hd::FoldScratch::bytes(n)))
		return HD_E_NOMEM;
	const hd::FoldScratch t(g.d_stream.p, n);
	uint32_t *carry = &t.w->v.check;
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)carry, kind == (int)hd::CHECK_ADLER32 ? 1 : 0, 1, st));
	if ((r = fold_launch((const uint32_t *)check, (const uint32_t *)len, n, (uint32_t)kind, t.tiles, t.prefix, t.w->fold, carry, st)))
		return r;
	HD_CHECK(hipMemcpyAsync(result, carry, 4, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	return 0;
}

// both forms of the stream: chunks that know nothing of each other (prime_max 0), or every chunk parsed with the
// min(prime_max, its offset) & ~1023 bytes in front of it as its history (levels 3..9; hipdeflate_stream_deflate_carry_dev)
static int stream_deflate_impl(const void *in, uint64_t nbytes, uint32_t chunk_bytes, int level, int frame, void *dst, uint64_t dst_cap,
			       void *chunk_off, hipdeflate_stream_summary *summary, void *stream, uint32_t prime_max)
{
	Ctx &g = cur();
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	if (!stream_frame_ok(frame) || !stream_chunk_ok(chunk_bytes) || ((uintptr_t)in & 15) || ((uintptr_t)dst & 15) || (nbytes && !in) ||
	    (dst_cap && !dst) || (nbytes + chunk_bytes - 1) / chunk_bytes > STREAM_MAX_PARTS)
		return HD_E_ARG;
	const uint32_t nchunks = (uint32_t)((nbytes + chunk_bytes - 1) / chunk_bytes);
	const uint32_t hdr = stream_hdr(frame), trl = stream_trl(frame);
	const uint32_t kind = frame == HD_FRAME_ZLIB ? hd::CHECK_ADLER32 : hd::CHECK_CRC32;
	const uint64_t slot = hipdeflate_bound(chunk_bytes, level);
	// a window of chunks: its slots total at most HD_STREAM_WINDOW_BYTES
	uint64_t W = g_test_stream_window ? g_test_stream_window : HD_STREAM_WINDOW_BYTES / slot;
	W = W < 1 ? 1 : W > nchunks ? (nchunks ? nchunks : 1) : W;
	if (!g_test_stream_window && nchunks)                          // windows of one size: no short one left over at the end
		W = (nchunks + (nchunks + W - 1) / W - 1) / ((nchunks + W - 1) / W);
	hipStream_t st = (hipStream_t)stream;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_stream.reserve(hd::EncodeWindow::bytes(W)) || (nchunks && g.d_stream_slots.reserve(W * slot + 16)))
		return HD_E_NOMEM;
	const hd::EncodeWindow t(g.d_stream.p, W);
	uint8_t *slots = (uint8_t *)g.d_stream_slots.p;
	uint32_t *carry = &t.w->v.check, *d_bad = &t.w->v.fault;     // the running check, the window's first bad chunk
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)carry, kind == hd::CHECK_ADLER32 ? 1 : 0, 1, st));
	uint64_t pos = hdr, bad_chunk = nchunks;
	bool fits = true;
	for (uint32_t c0 = 0; c0 < nchunks; c0 += (uint32_t)W) {
		const uint32_t w = nchunks - c0 < W ? nchunks - c0 : (uint32_t)W, wgs = (w + 255) / 256;
		hipLaunchKernelGGL(hd::k_stream_table, dim3(wgs), dim3(256), 0, st, c0, w, chunk_bytes, nbytes, t.in_off, t.in_len);
		// (k_stream_table's offsets are relative to `in` in every window: a window's first chunk is primed like any other)
		if ((r = batch_deflate_dev_impl(in, t.in_off, t.in_len, w, level, HD_FRAME_RAW_FLUSH, slots, slot, (uint32_t)slot, t.out_len, t.crc,
						t.status, stream, 0, prime_max)))
			return r;
		// every chunk's place in the stream, straight into the caller's table where there is one: the running total goes
		// from window to window as the scan's base
		uint64_t *dst_off = chunk_off ? (uint64_t *)chunk_off + c0 : t.own_off;
		index_scan(t.out_len, w, t.tiles, dst_off, &t.w->total, st, pos);
		HD_CHECK(hipMemsetAsync(d_bad, 0xff, 4, st));
		hipLaunchKernelGGL(hd::k_members_verify, dim3(wgs), dim3(256), 0, st, (const int32_t *)t.status, (const uint32_t *)t.out_len,
				   (const uint32_t *)t.crc, (const uint32_t *)t.out_len, (const uint32_t *)t.crc, w, d_bad);     // (the status alone)
		if (kind == hd::CHECK_ADLER32)
			hipLaunchKernelGGL(hd::k_chunk_adler, dim3(w), dim3(64), 0, st, (const uint8_t *)in, (const uint64_t *)t.in_off,
					   (const uint32_t *)t.in_len, (const uint32_t *)nullptr, w, t.adler);
		if ((r = fold_launch(kind == hd::CHECK_ADLER32 ? t.adler : t.crc, t.in_len, w, kind, t.tiles, t.prefix, t.w->fold, carry, st)))
			return r;
		hd::StreamWords h;
		HD_CHECK(hipMemcpyAsync(&h, t.w, offsetof(hd::StreamWords, v.mismatch), hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
		if (h.v.fault != hd::IDX_NIL && bad_chunk == nchunks)
			bad_chunk = (uint64_t)c0 + h.v.fault;
		// the gather, the scan's base as the header and the windows in front: only while every byte of it has room
		if (fits && pos + h.total <= dst_cap)
			hd::launch_compact(slots, slot, t.out_len, dst_off, w, (uint8_t *)dst, st);
		else
			fits = false;
		pos += h.total;
	}
	const uint64_t need = pos + 2 + trl;
	fits = fits && need <= dst_cap;
	if (fits)
		hipLaunchKernelGGL(hd::k_stream_ends, dim3(1), dim3(64), 0, st, (uint8_t *)dst, frame, pos, (const uint32_t *)carry,
				   (uint32_t)nbytes, chunk_off ? (uint64_t *)chunk_off + nchunks : (uint64_t *)nullptr);
	else if (chunk_off)
		HD_CHECK(hipMemcpyAsync((uint64_t *)chunk_off + nchunks, &pos, 8, hipMemcpyHostToDevice, st));
	HD_CHECK(hipGetLastError());
	uint32_t check = 0;
	HD_CHECK(hipMemcpyAsync(&check, carry, 4, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	summary->out_bytes = need;
	summary->in_bytes = nbytes;
	summary->bad_chunk = bad_chunk;
	summary->nchunks = nchunks;
	summary->check = check;
	summary->status = bad_chunk != nchunks ? 2u : fits ? 0u : 3u;
	return 0;
}

int hipdeflate_stream_deflate_dev(const void *in, uint64_t nbytes, uint32_t chunk_bytes, int level, int frame, void *dst,
				  uint64_t dst_cap, void *chunk_off, hipdeflate_stream_summary *summary, void *stream)
{
	return stream_deflate_impl(in, nbytes, chunk_bytes, level, frame, dst, dst_cap, chunk_off, summary, stream, 0);
}

int hipdeflate_stream_deflate_carry_dev(const void *in, uint64_t nbytes, uint32_t chunk_bytes, int level, int frame, void *dst,
					uint64_t dst_cap, void *chunk_off, hipdeflate_stream_summary *summary, void *stream)
{
	return stream_deflate_impl(in, nbytes, chunk_bytes, level, frame, dst, dst_cap, chunk_off, summary, stream, HD_WG_WINDOW);
}

// a row table as a decoder takes it: the caller's columns, or (the decode by chunk table) the scratch's own
struct StreamRows {
	const uint64_t *in_off;
	const uint32_t *in_len;
	const uint64_t *out_off;
	const uint32_t *out_size, *reach;        // reach: the carry decode's
};

// the verdict words before a decode: the check's start value, no fault, no bad row
static int stream_words_reset(hd::StreamWords *w, uint32_t kind, hipStream_t st)
{
	HD_CHECK(hipMemsetAsync(w, 0, sizeof *w, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&w->v.check, kind == hd::CHECK_ADLER32 ? 1 : 0, 1, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&w->v.fault, (int)hd::IDX_NIL, 1, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&w->v.bad, (int)hd::IDX_NIL, 1, st));
	return 0;
}

// Rows [r0, r0 + nr) by the flush rule: row i inflated into out + out_off[i] with out_size[i] as room and held to its size
// (status and length; the lowest row that fails -> v.bad), the rows' checks folded onto v.check
static int stream_rows_flushed(Ctx &g, const void *strm, uint32_t kind, const StreamRows &t, const hd::DecodeScratch &d, uint32_t r0,
			       uint32_t nr, void *out, hipStream_t st)
{
	int r;
	if (nr) {
		if ((r = launch_inflate({ (const uint8_t *)strm, t.in_off + r0, t.in_len + r0, nr, (uint8_t *)out, t.out_off + r0, t.out_size + r0,
					  d.out_len + r0, kind == hd::CHECK_ADLER32 ? nullptr : d.chk + r0, d.status + r0, g.d_ct, hd::INF_FLUSHED },
					st)))
			return r;
		if (kind == hd::CHECK_ADLER32)
			hipLaunchKernelGGL(hd::k_chunk_adler, dim3(nr), dim3(64), 0, st, (const uint8_t *)out, t.out_off + r0,
					   (const uint32_t *)(d.out_len + r0), t.out_size + r0, nr, d.chk + r0);
		hipLaunchKernelGGL(hd::k_carry_verify, dim3((nr + 255) / 256), dim3(256), 0, st, (const int32_t *)d.status,
				   (const uint32_t *)d.out_len, t.out_size, r0, nr, &d.w->v.bad);
	}
	return fold_launch(d.chk + r0, t.out_size + r0, nr, kind, d.tiles, d.prefix, d.w->fold, &d.w->v.check, st);
}

// The end of a decode: the folded check held to the trailer that ends at in_bytes, the verdict read, the summary filled
// (the caller has set summary->nchunks and bad_chunk)
static int stream_decode_end(const void *strm, uint64_t in_bytes, int frame, uint64_t out_bytes, hd::StreamWords *w,
			     hipdeflate_stream_summary *summary, hipStream_t st)
{
	hipLaunchKernelGGL(hd::k_stream_trailer, dim3(1), dim3(64), 0, st, (const uint8_t *)strm, in_bytes, frame, out_bytes,
			   (const uint32_t *)&w->v.check, &w->v.mismatch);
	HD_CHECK(hipGetLastError());
	hd::StreamVerdict h;
	HD_CHECK(hipMemcpyAsync(&h, &w->v, sizeof h, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	summary->out_bytes = out_bytes;
	summary->in_bytes = in_bytes;
	summary->check = h.check;
	if (h.bad != hd::IDX_NIL || h.mismatch)
		summary->status = 2;
	if (h.bad != hd::IDX_NIL)
		summary->bad_chunk = h.bad;
	return 0;
}

/* ---- ... and a stream nobody kept a table for: the index of its flush points (hd_stream.hpp) ---- */

// The header of the stream by k_frame_open's rules, on the first min(nbytes, HD_INFLATE_MAX_IN - 1) bytes: *hdr its length.
// -> 0, 1 the rules refuse it, 2 nbytes is below the frame's header and trailer.  w: eight u64 of device scratch.
// (Synchronises the stream.)
static int stream_open(const void *strm, uint64_t nbytes, int frame, uint64_t *w, hipStream_t st, uint32_t *hdr, uint32_t *verdict)
{
	*hdr = 0;
	*verdict = 0;
	if (frame == HD_FRAME_RAW)
		return 0;
	if (nbytes < (frame == HD_FRAME_GZIP ? 18u : 6u)) {
		*verdict = 2;
		return 0;
	}
	// w[0] the member's offset | w[1] its payload's | w[2] as u32: the member's length, the payload's | w[3] as i32: the verdict
	const uint32_t n = nbytes < HD_INFLATE_MAX_IN ? (uint32_t)nbytes : HD_INFLATE_MAX_IN - 1;
	HD_CHECK(hipMemsetAsync(w, 0, 32, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)(w + 2), (int)n, 1, st));
	hipLaunchKernelGGL(hd::k_frame_open, dim3(1), dim3(64), 0, st, (const uint8_t *)strm, (const uint64_t *)w, (const uint32_t *)(w + 2), 1u,
			   frame, w + 1, (uint32_t *)(w + 2) + 1, (int32_t *)(w + 3));
	HD_CHECK(hipGetLastError());
	uint64_t h[4];
	HD_CHECK(hipMemcpyAsync(h, w, 32, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if ((uint32_t)h[3])
		*verdict = 1;
	else
		*hdr = (uint32_t)h[1];
	return 0;
}

// own: the tables are the library's, made as large as the stream needs once that is known -- a hd::RowTable of the chain's
// rows (summary->nchunks where the status is 0) in *own -- and the table arguments are not looked at.  carry: the index
// of hd_carry.hpp -- k_carry_piece in the place of k_inflate_piece, the reach column, and the reach rule behind the verdict.
static int stream_index(Ctx &g, const void *strm, uint64_t nbytes, int frame, uint32_t max_chunks, uint32_t max_chunk_in, void *in_off,
			void *in_len, void *out_size, void *out_off, hipdeflate_stream_index_summary *summary, hipStream_t st, Buf *own,
			bool carry = false, void *reach = nullptr)
{
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	if (!stream_frame_ok(frame) || ((uintptr_t)strm & 15) || (nbytes && !strm) || max_chunk_in >= HD_INFLATE_MAX_IN ||
	    (max_chunks && (!in_off || !in_len || !out_size || !out_off || (carry && !reach))))
		return HD_E_ARG;
	const uint8_t *src = (const uint8_t *)strm;
	const uint32_t trl = stream_trl(frame);
	if (max_chunk_in == 0)
		max_chunk_in = HD_INFLATE_MAX_IN - 1;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_index.reserve(hd::IndexBitmap::bytes(0, 0, true)))
		return HD_E_NOMEM;
	uint32_t hdr = 0, refused = 0;
	if ((r = stream_open(strm, nbytes, frame, hd::IndexBitmap(g.d_index.p, 0, 0, true).header, st, &hdr, &refused)))
		return r;
	summary->hdr_bytes = hdr;
	summary->end_offset = hdr;
	if (refused) {
		summary->status = refused;
		return 0;
	}
	summary->ncandidates = 1;                                                // the first payload byte, whatever it is
	const uint64_t payload_end = nbytes - trl;                               // (k_frame_open: hdr + trl <= nbytes)
	if (payload_end == hdr) {
		summary->status = 2;
		return 0;
	}
	// the passes' nbytes is the last payload byte: a marker there makes no candidate
	hd::IndexWords *w = nullptr;
	hd::IndexCand c;
	uint32_t ncand = 0;
	r = chain_candidates(g, src, payload_end - 1, &hdr, carry ? hd::INDEX_CARRY : hd::INDEX_STREAM, 0, w, c, ncand, st);
	if (ncand)
		summary->ncandidates = ncand;
	if (r)
		return r;
	const uint32_t nwg = (ncand + 255) / 256;
	// one bounded decode per candidate
	if (carry)
		hipLaunchKernelGGL(hd::k_carry_piece, dim3(ncand), dim3(64), 0, st,
				   hd::CarryPieceArgs{ { src, (const uint64_t *)c.pos, ncand, max_chunk_in, payload_end, c.osize, c.used, c.pstat, c.stop },
						       c.reach });
	else
		hipLaunchKernelGGL(hd::k_inflate_piece, dim3(ncand), dim3(64), 0, st,
				   hd::PieceArgs{ src, (const uint64_t *)c.pos, ncand, max_chunk_in, payload_end, c.osize, c.used, c.pstat, c.stop });
	hipLaunchKernelGGL(hd::k_stream_links, dim3(nwg), dim3(256), 0, st, (const uint64_t *)c.pos, (const uint32_t *)c.used,
			   (const uint32_t *)c.stop, ncand, c.succ0, c.mark);
	uint64_t nrows = 0;
	if ((r = chain_rank(c, ncand, c.used, w, &nrows, st)))
		return r;
	if (own) {
		if (own->reserve(hd::RowTable::bytes(nrows, carry)))
			return HD_E_NOMEM;
		const hd::RowTable t(own->p, nrows, carry);
		max_chunks = (uint32_t)nrows;
		in_off = t.in_off, out_off = t.out_off, in_len = t.in_len, out_size = t.out_size, reach = t.reach;
	}
	const uint32_t ntab = (uint32_t)(nrows < max_chunks ? nrows : max_chunks);
	if (nrows) {
		hipLaunchKernelGGL(hd::k_stream_rows, dim3(nwg), dim3(256), 0, st, (const uint64_t *)c.pos, (const uint32_t *)c.used,
				   (const uint32_t *)c.osize, (const uint32_t *)c.mark, (const uint64_t *)c.rank, ncand, nrows, max_chunks,
				   (uint64_t *)in_off, (uint32_t *)in_len, (uint32_t *)out_size, &w->last);
		if (ntab)
			index_scan((const uint32_t *)out_size, ntab, c.tiles, (uint64_t *)out_off, &w->out_bytes, st);
		if (carry && ntab)
			hipLaunchKernelGGL(hd::k_carry_reach_rows, dim3(nwg), dim3(256), 0, st, (const uint32_t *)c.reach, (const uint32_t *)c.mark,
					   (const uint64_t *)c.rank, ncand, max_chunks, (uint32_t *)reach);
	}
	hipLaunchKernelGGL(hd::k_stream_verdict, dim3(1), dim3(1), 0, st, (const uint64_t *)c.pos, (const uint32_t *)c.used,
			   (const int32_t *)c.pstat, (const uint32_t *)c.stop, ncand, nrows, max_chunks, max_chunk_in, payload_end, trl, &w->rows);
	if (carry && ntab) {
		// the reach rule, on the rows in the table: w->first = the first row that reaches back over the stream's start
		HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&w->first, (int)hd::IDX_NIL, 1, st));
		hipLaunchKernelGGL(hd::k_carry_check_reach, dim3((ntab + 255) / 256), dim3(256), 0, st, (const uint32_t *)reach,
				   (const uint64_t *)out_off, ntab, 0xffffffffu, &w->first);
		hipLaunchKernelGGL(hd::k_carry_cut, dim3(1), dim3(64), 0, st, (const uint32_t *)&w->first, (const uint64_t *)in_off,
				   (const uint64_t *)out_off, &w->rows);
	}
	return chain_read(w, &summary->nchunks, &summary->out_bytes, &summary->end_offset, &summary->status, st);
}

int hipdeflate_stream_index_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_chunks, uint32_t max_chunk_in, void *in_off,
				void *in_len, void *out_size, void *out_off, hipdeflate_stream_index_summary *summary, void *stream)
{
	return stream_index(cur(), strm, nbytes, frame, max_chunks, max_chunk_in, in_off, in_len, out_size, out_off, summary,
			    (hipStream_t)stream, nullptr);
}

/* ---- ... and a stream cut by sync flushes, which carry the window across the cut (hd_carry.hpp) ---- */

static uint64_t g_test_carry_group = 0;                       // hipdeflate_test_carry_group
void hipdeflate_test_carry_group(uint64_t bytes) { g_test_carry_group = bytes; }

// hipdeflate_test_carry_times: milliseconds of the marker path's passes -- decode, tails, resolve, check and fold -- by
// events around the launches of every group, while it is on (tools/stream_carry_bench.py)
static bool g_carry_timed = false;
static double g_carry_ms[4] = { 0, 0, 0, 0 };
void hipdeflate_test_carry_times(double *ms4)
{
	for (int k = 0; k < 4; k++) {
		if (ms4)
			ms4[k] = g_carry_ms[k];
		g_carry_ms[k] = 0;
	}
	g_carry_timed = ms4 != nullptr;
}
struct CarryTimer {
	hipEvent_t ev[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
	bool on;
	explicit CarryTimer(bool on_) : on(on_)
	{
		for (int k = 0; on && k < 5; k++)
			if (hipEventCreate(&ev[k]) != hipSuccess)
				on = false;
	}
	void mark(int k, hipStream_t st)
	{
		if (on)
			(void)hipEventRecord(ev[k], st);
	}
	void add(double *ms)
	{
		if (!on || hipEventSynchronize(ev[4]) != hipSuccess)
			return;
		for (int k = 0; k < 4; k++) {
			float t = 0;
			if (hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess)
				ms[k] += t;
		}
	}
	~CarryTimer()
	{
		for (int k = 0; k < 5; k++)
			if (ev[k])
				(void)hipEventDestroy(ev[k]);
	}
};

int hipdeflate_stream_index_carry_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_chunks, uint32_t max_chunk_in, void *in_off,
				      void *in_len, void *out_size, void *out_off, void *reach, hipdeflate_stream_index_summary *summary,
				      void *stream)
{
	return stream_index(cur(), strm, nbytes, frame, max_chunks, max_chunk_in, in_off, in_len, out_size, out_off, summary,
			    (hipStream_t)stream, nullptr, true, reach);
}

// The carry decode's rows, group by group in stream order: the check runs on in d.w->v.check, the lowest bad row in v.bad.
// bits: the rows of the block index (hd_blocks.hpp), which start and end on a bit -- every group takes the marker path
static int carry_decode_groups(Ctx &g, const void *strm, uint32_t kind, const StreamRows &t, const hd::DecodeScratch &d, uint32_t nchunks,
			       void *out, hipStream_t st, bool bits = false)
{
	int r;
	uint32_t *carry = &d.w->v.check, *d_bad = &d.w->v.bad;
	const uint64_t group_bytes = g_test_carry_group ? g_test_carry_group : HD_CARRY_GROUP_BYTES;
	for (uint32_t r0 = 0; r0 < nchunks;) {
		uint64_t gr[4];
		hd::StreamVerdict h;
		hipLaunchKernelGGL(hd::k_carry_group, dim3(1), dim3(256), 0, st, t.out_off, t.out_size, t.reach, r0, nchunks, group_bytes, d.group);
		HD_CHECK(hipGetLastError());
		HD_CHECK(hipMemcpyAsync(gr, d.group, 32, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipMemcpyAsync(&h, &d.w->v, sizeof h, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
		if (h.bad != hd::IDX_NIL)
			break;                                                    // a row of an earlier group is bad: the verdict is in
		const uint32_t r1 = (uint32_t)gr[0], nr = r1 - r0;
		const uint64_t begin = gr[2], gbytes = gr[3] - gr[2];
		if (gr[1] == 0 && !bits) {                                        // no row of the group reaches back
			if ((r = stream_rows_flushed(g, strm, kind, t, d, r0, nr, out, st)))
				return r;
		} else {
			// the marker path: the group as symbols, and its check in pieces
			const uint64_t np64 = (gbytes + HD_CARRY_CHECK_PIECE - 1) / HD_CARRY_CHECK_PIECE;
			if (np64 >= STREAM_MAX_PARTS || gbytes > (uint64_t)1 << 40 ||
			    g.d_stream_slots.reserve(hd::MarkerScratch::bytes(gbytes, np64)))
				return HD_E_NOMEM;
			const uint32_t np = (uint32_t)np64;
			const hd::MarkerScratch m(g.d_stream_slots.p, gbytes, np);
			CarryTimer tm(g_carry_timed);
			tm.mark(0, st);
			const hd::CarryDecodeArgs da{ (const uint8_t *)strm, t.in_off, t.in_len, t.out_size, t.out_off, t.reach, r0, nr, begin,
						      m.sym, d.out_len, d.status };
			if (bits)
				hipLaunchKernelGGL(hd::k_blocks_decode, dim3(nr), dim3(64), 0, st, hd::BlocksDecodeArgs{ da });
			else
				hipLaunchKernelGGL(hd::k_carry_decode, dim3(nr), dim3(64), 0, st, da);
			const hd::CarryRowsArgs ra{ m.sym, begin, t.out_off, t.out_size, d.out_len, d.status, r0, nr, (uint8_t *)out };
			tm.mark(1, st);
			hipLaunchKernelGGL(hd::k_carry_tails, dim3(1), dim3(hd::CARRY_TAIL_THREADS), 0, st, ra);
			tm.mark(2, st);
			hipLaunchKernelGGL(hd::k_carry_resolve, dim3(nr), dim3(256), 0, st, ra);
			tm.mark(3, st);
			hipLaunchKernelGGL(hd::k_carry_verify, dim3((nr + 255) / 256), dim3(256), 0, st, (const int32_t *)d.status,
					   (const uint32_t *)d.out_len, t.out_size, r0, nr, d_bad);
			if (np) {
				hipLaunchKernelGGL(hd::k_carry_parts, dim3((np + 255) / 256), dim3(256), 0, st, begin, gr[3], np, m.off, m.len);
				if (kind == hd::CHECK_ADLER32)
					hipLaunchKernelGGL(hd::k_chunk_adler, dim3(np), dim3(64), 0, st, (const uint8_t *)out, (const uint64_t *)m.off,
							   (const uint32_t *)m.len, (const uint32_t *)nullptr, np, m.chk);
				else
					hipLaunchKernelGGL(hd::k_carry_crc, dim3(np), dim3(64), 0, st, (const CrcTables *)g.d_ct, (const uint8_t *)out,
							   (const uint64_t *)m.off, (const uint32_t *)m.len, np, m.chk);
				if ((r = fold_launch(m.chk, m.len, np, kind, m.tiles, m.prefix, d.w->fold, carry, st)))
					return r;
			}
			tm.mark(4, st);
			tm.add(g_carry_ms);
		}
		r0 = r1;
	}
	return 0;
}

// The three decoders behind their entry points.  By rows: the caller's table t held to the stream's rules (carry: and its
// reach column), the trailer behind the last row wherever the caller's buffer ends.  By chunks (ct): the rows made from the
// chunk table by k_stream_check_table, the trailer at the buffer's end.  Then the rows decoded -- side by side by the flush
// rule, or group by group -- and the folded check held to the trailer.
struct StreamChunks {
	const uint64_t *off;
	uint32_t bytes;
	uint64_t out_bytes;
};
// bits (with carry): the block index's table, in_off and in_len in bits (k_blocks_check_rows, k_blocks_decode).
static int stream_inflate_rows(Ctx &g, const void *strm, uint64_t nbytes, int frame, StreamRows t, const StreamChunks *ct, bool carry,
			       uint32_t nchunks, void *out, uint64_t out_cap, hipdeflate_stream_summary *summary, hipStream_t st,
			       bool bits = false)
{
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	summary->bad_chunk = summary->nchunks = nchunks;
	if (!stream_frame_ok(frame) || ((uintptr_t)strm & 15) || (nbytes && !strm) || nchunks >= STREAM_MAX_PARTS || (out_cap && !out) ||
	    (ct ? !stream_chunk_ok(ct->bytes) || !ct->off
		: nchunks && (!t.in_off || !t.in_len || !t.out_size || !t.out_off || (carry && !t.reach))))
		return HD_E_ARG;
	const uint32_t trl = stream_trl(frame), kind = frame == HD_FRAME_ZLIB ? hd::CHECK_ADLER32 : hd::CHECK_CRC32;
	// before any byte is looked at, and before the lock.  By chunks: what nchunks and the chunk size allow, a stream long
	// enough for its two ends.  By rows: a stream has its final block, and that is a row
	if (ct ? (ct->out_bytes + ct->bytes - 1) / ct->bytes != nchunks || nbytes < (uint64_t)stream_hdr(frame) + 2 + trl : nchunks == 0) {
		summary->status = 1;
		return 0;
	}
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_stream.reserve(hd::DecodeScratch::bytes(nchunks, ct != nullptr)))
		return HD_E_NOMEM;
	const hd::DecodeScratch d(g.d_stream.p, nchunks, ct != nullptr);
	uint32_t hdr = 0, refused = 0;
	if (!ct && (r = stream_open(strm, nbytes, frame, d.header, st, &hdr, &refused)))
		return r;
	if (refused) {
		summary->status = 1;
		return 0;
	}
	if ((r = stream_words_reset(d.w, kind, st)))
		return r;
	uint64_t e[2] = { nbytes - trl, ct ? ct->out_bytes : 0 };     // where the rows end: in the stream, in the output
	if (ct) {
		hipLaunchKernelGGL(hd::k_stream_check_table, dim3((nchunks + 1 + 255) / 256), dim3(256), 0, st, (const uint8_t *)strm, nbytes,
				   ct->off, nchunks, ct->bytes, ct->out_bytes, frame, d.in_off, d.in_len, d.out_off, d.out_size, &d.w->v.fault);
		t = { d.in_off, d.in_len, d.out_off, d.out_size, nullptr };
	} else {
		HD_CHECK(hipMemsetAsync(d.ends, 0, 16, st));
		if (bits)
			hipLaunchKernelGGL(hd::k_blocks_check_rows, dim3((nchunks + 255) / 256), dim3(256), 0, st, t.in_off, t.in_len, t.out_size,
					   t.out_off, nchunks, (uint64_t)hdr, nbytes - trl, &d.w->v.fault, d.ends);
		else
			hipLaunchKernelGGL(hd::k_stream_check_rows, dim3((nchunks + 255) / 256), dim3(256), 0, st, t.in_off, t.in_len, t.out_size,
					   t.out_off, nchunks, (uint64_t)hdr, nbytes - trl, &d.w->v.fault, d.ends);
		if (carry)
			hipLaunchKernelGGL(hd::k_carry_check_reach, dim3((nchunks + 255) / 256), dim3(256), 0, st, t.reach, t.out_off, nchunks,
					   hd::CARRY_WINDOW, &d.w->v.fault);
	}
	HD_CHECK(hipGetLastError());
	hd::StreamVerdict h;
	HD_CHECK(hipMemcpyAsync(&h, &d.w->v, sizeof h, hipMemcpyDeviceToHost, st));
	if (!ct)
		HD_CHECK(hipMemcpyAsync(e, d.ends, 16, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (h.fault != hd::IDX_NIL) {
		summary->status = 1;
		summary->bad_chunk = h.fault;
		return 0;
	}
	if (out_cap < e[1]) {
		summary->status = 3;
		summary->out_bytes = ct ? 0 : e[1];
		return 0;
	}
	if ((r = carry ? carry_decode_groups(g, strm, kind, t, d, nchunks, out, st, bits) : stream_rows_flushed(g, strm, kind, t, d, 0, nchunks, out, st)))
		return r;
	return stream_decode_end(strm, (bits ? (e[0] + 7) >> 3 : e[0]) + trl, frame, e[1], d.w, summary, st);
}

int hipdeflate_stream_inflate_dev(const void *strm, uint64_t nbytes, int frame, const void *chunk_off, uint32_t nchunks,
				  uint32_t chunk_bytes, uint64_t out_bytes, void *out, uint64_t out_cap,
				  hipdeflate_stream_summary *summary, void *stream)
{
	const StreamChunks ct = { (const uint64_t *)chunk_off, chunk_bytes, out_bytes };
	return stream_inflate_rows(cur(), strm, nbytes, frame, {}, &ct, false, nchunks, out, out_cap, summary, (hipStream_t)stream);
}

int hipdeflate_stream_inflate_table_dev(const void *strm, uint64_t nbytes, int frame, const void *in_off, const void *in_len,
					const void *out_size, const void *out_off, uint32_t nchunks, void *out, uint64_t out_cap,
					hipdeflate_stream_summary *summary, void *stream)
{
	return stream_inflate_rows(cur(), strm, nbytes, frame,
				   { (const uint64_t *)in_off, (const uint32_t *)in_len, (const uint64_t *)out_off, (const uint32_t *)out_size, nullptr },
				   nullptr, false, nchunks, out, out_cap, summary, (hipStream_t)stream);
}

int hipdeflate_stream_inflate_carry_dev(const void *strm, uint64_t nbytes, int frame, const void *in_off, const void *in_len,
					const void *out_size, const void *out_off, const void *reach, uint32_t nchunks, void *out,
					uint64_t out_cap, hipdeflate_stream_summary *summary, void *stream)
{
	const StreamRows t = { (const uint64_t *)in_off, (const uint32_t *)in_len, (const uint64_t *)out_off, (const uint32_t *)out_size,
			       (const uint32_t *)reach };
	return stream_inflate_rows(cur(), strm, nbytes, frame, t, nullptr, true, nchunks, out, out_cap, summary, (hipStream_t)stream);
}

/* ---- ... and a stream without a flush point: the index of its blocks, rows that start and end on a bit (hd_blocks.hpp) ---- */

// hipdeflate_test_blocks_times: milliseconds of the index's passes -- candidates, pieces, chain, merge (tools/stream_blocks_bench.py)
static bool g_blocks_timed = false;
static double g_blocks_ms[4] = { 0, 0, 0, 0 };
void hipdeflate_test_blocks_times(double *ms4)
{
	for (int k = 0; k < 4; k++) {
		if (ms4)
			ms4[k] = g_blocks_ms[k];
		g_blocks_ms[k] = 0;
	}
	g_blocks_timed = ms4 != nullptr;
}

// hipdeflate_test_blocks_counts: of the last index call made while the timing was on, the candidates whose piece got past its
// own first block header, and those whose piece decodes to its stop
static uint64_t g_blocks_counts[2] = { 0, 0 };
void hipdeflate_test_blocks_counts(uint64_t *out2)
{
	out2[0] = g_blocks_counts[0];
	out2[1] = g_blocks_counts[1];
}

// The candidate list of src[0, end): `first`, a bit position, whatever stands there, then every position behind it that passes
// the header rule (k_blocks_flag, k_blocks_write), ascending, in c.pos.  header8: eight dead u64 of d_index.  (Synchronises.)
static int blocks_candidates(Ctx &g, const uint8_t *src, uint64_t end, uint64_t first, hd::IndexWords *&w, hd::IndexCand &c,
			     uint32_t &ncand, uint64_t *&header8, hipStream_t st)
{
	const uint64_t nwords = (end + hd::IDX_WORD - 1) / hd::IDX_WORD, ntb64 = (nwords + hd::BLOCK_TILE_WORDS - 1) / hd::BLOCK_TILE_WORDS;
	if (ntb64 > 0x7fffffffu)
		return HD_E_ARG;
	const uint32_t ntb = (uint32_t)ntb64;
	if (g.d_index.reserve(hd::IndexBitmap::bytes(ntb, nwords, true)))
		return HD_E_NOMEM;
	const hd::IndexBitmap b(g.d_index.p, ntb, nwords, true);
	w = b.w;
	header8 = b.header;
	uint64_t found = 0;
	HD_CHECK(hipMemsetAsync(w, 0, sizeof *w, st));
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&w->first, (int)hd::IDX_NIL, 1, st));
	hipLaunchKernelGGL(hd::k_blocks_flag, dim3(ntb), dim3(64), 0, st, src, end, first + 1, b.bitmap, b.tile_cnt);
	index_scan(b.tile_cnt, ntb, b.tiles, b.tile_off, &w->ncand, st);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&found, &w->ncand, 8, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (found + 1 > 0x7fffffffu)
		return HD_E_NOMEM;
	ncand = (uint32_t)found + 1;
	if (g.d_cand.reserve(hd::IndexCand::bytes(ncand, 0, hd::INDEX_BLOCKS)))
		return HD_E_NOMEM;
	c = hd::IndexCand(g.d_cand.p, ncand, 0, hd::INDEX_BLOCKS);
	HD_CHECK(hipMemcpyAsync(c.pos, &first, 8, hipMemcpyHostToDevice, st));
	HD_CHECK(hipStreamSynchronize(st));                                      // (`first` is the caller's)
	if (ncand > 1)
		hipLaunchKernelGGL(hd::k_blocks_write, dim3(ntb), dim3(64), 0, st, src, end, first + 1, (const uint64_t *)b.bitmap, nwords,
				   (const uint64_t *)b.tile_off, c.pos + 1);
	return 0;
}

int hipdeflate_test_block_candidates_dev(const void *strm, uint64_t nbytes, uint64_t first, void *pos, uint32_t max_pos, uint64_t *count,
					 void *stream)
{
	Ctx &g = cur();
	const int e = ensure();
	if (e)
		return e;
	if (!strm || !nbytes || ((uintptr_t)strm & 15) || nbytes > ((uint64_t)1 << 60) || first >= 8 * nbytes || !count || (max_pos && !pos))
		return HD_E_ARG;
	hipStream_t st = (hipStream_t)stream;
	std::lock_guard<std::mutex> lk(g.mu_index);
	hd::IndexWords *w = nullptr;
	hd::IndexCand c;
	uint32_t ncand = 0;
	uint64_t *unused = nullptr;
	int r = blocks_candidates(g, (const uint8_t *)strm, nbytes, first, w, c, ncand, unused, st);
	if (r)
		return r;
	*count = ncand;
	const uint32_t n = ncand < max_pos ? ncand : max_pos;
	if (n)
		HD_CHECK(hipMemcpyAsync(pos, c.pos, 8 * (size_t)n, hipMemcpyDeviceToDevice, st));
	HD_CHECK(hipStreamSynchronize(st));
	return 0;
}

int hipdeflate_test_block_headers_dev(const void *strm, uint64_t nbytes, const void *pos, uint32_t n, void *verdict, void *stream)
{
	const int r = ensure();
	if (r)
		return r;
	if ((nbytes && !strm) || nbytes > ((uint64_t)1 << 60) || (n && (!pos || !verdict)))
		return HD_E_ARG;
	if (n)
		hipLaunchKernelGGL(hd::k_blocks_rule, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const uint8_t *)strm, nbytes,
				   (const uint64_t *)pos, n, (uint32_t *)verdict);
	HD_CHECK(hipGetLastError());
	return 0;
}

// own: as stream_index has it -- a hd::RowTable with the reach column in *own, as large as the chain needs
static int blocks_index(Ctx &g, const void *strm, uint64_t nbytes, int frame, uint32_t max_rows, uint32_t max_chunk_in, uint32_t row_bytes,
			void *in_off, void *in_len, void *out_size, void *out_off, void *reach, hipdeflate_block_index_summary *summary,
			hipStream_t st, Buf *own)
{
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	if (!stream_frame_ok(frame) || ((uintptr_t)strm & 15) || (nbytes && !strm) || max_chunk_in >= HD_INFLATE_MAX_IN ||
	    (max_rows && (!in_off || !in_len || !out_size || !out_off || !reach)))
		return HD_E_ARG;
	const uint8_t *src = (const uint8_t *)strm;
	const uint32_t trl = stream_trl(frame);
	if (max_chunk_in == 0)
		max_chunk_in = HD_INFLATE_MAX_IN - 1;
	if (row_bytes == 0)
		row_bytes = HD_BLOCK_ROW_BYTES;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_index.reserve(hd::IndexBitmap::bytes(0, 0, true)))
		return HD_E_NOMEM;
	uint32_t hdr = 0, refused = 0;
	if ((r = stream_open(strm, nbytes, frame, hd::IndexBitmap(g.d_index.p, 0, 0, true).header, st, &hdr, &refused)))
		return r;
	summary->hdr_bytes = hdr;
	summary->end_offset = hdr;
	summary->end_bit = 8 * (uint64_t)hdr;
	if (refused) {
		summary->status = refused;
		return 0;
	}
	summary->ncandidates = 1;                                                // the first payload bit, whatever stands there
	const uint64_t payload_end = nbytes - trl;                               // (k_frame_open: hdr + trl <= nbytes)
	if (payload_end == hdr) {
		summary->status = 2;
		return 0;
	}
	hd::IndexWords *w = nullptr;
	hd::IndexCand c;
	uint32_t ncand = 0;
	uint64_t *counts = nullptr;
	CarryTimer tm(g_blocks_timed);
	tm.mark(0, st);
	if ((r = blocks_candidates(g, src, payload_end, 8 * (uint64_t)hdr, w, c, ncand, counts, st)))
		return r;
	const uint32_t nwg = (ncand + 255) / 256;
	summary->ncandidates = ncand;
	tm.mark(1, st);
	// one bounded decode per candidate, from its bit
	hipLaunchKernelGGL(hd::k_blocks_piece, dim3(ncand), dim3(64), 0, st,
			   hd::BlocksPieceArgs{ { { src, (const uint64_t *)c.pos, ncand, max_chunk_in, payload_end, c.osize, c.used, c.pstat, c.stop },
						c.reach } });
	tm.mark(2, st);
	if (g_blocks_timed) {                                                    // (the bench's two counts, in the header's dead words)
		HD_CHECK(hipMemsetAsync(counts, 0, 16, st));
		hipLaunchKernelGGL(hd::k_blocks_count, dim3(nwg), dim3(256), 0, st, (const uint32_t *)c.stop, (const uint32_t *)c.used, ncand,
				   (unsigned long long *)counts);
		HD_CHECK(hipMemcpyAsync(g_blocks_counts, counts, 16, hipMemcpyDeviceToHost, st));
	}
	hipLaunchKernelGGL(hd::k_blocks_links, dim3(nwg), dim3(256), 0, st, (const uint64_t *)c.pos, (const uint32_t *)c.used,
			   (const uint32_t *)c.stop, ncand, c.succ0, c.mark);
	uint64_t npieces = 0, nrows = 0;
	if ((r = chain_rank(c, ncand, c.used, w, &npieces, st)))
		return r;
	tm.mark(3, st);
	// the merge: the chain's pieces in rank order, the rows they begin, the rows' columns
	const uint64_t *h_pos = nullptr, *h_out = nullptr;
	if (npieces) {
		const uint32_t np = (uint32_t)npieces, npg = (np + 255) / 256;
		if (g.d_blocks.reserve(hd::BlockPieces::bytes(np)))
			return HD_E_NOMEM;
		const hd::BlockPieces m(g.d_blocks.p, np);
		h_pos = m.h_pos, h_out = m.h_out;
		hipLaunchKernelGGL(hd::k_blocks_sizes, dim3(nwg), dim3(256), 0, st, (const uint32_t *)c.osize, (const uint32_t *)c.mark,
				   (const uint64_t *)c.rank, ncand, npieces, m.p_size, &w->last);
		index_scan(m.p_size, np, m.tiles, m.p_out, &w->out_bytes, st);
		hipLaunchKernelGGL(hd::k_blocks_starts, dim3(npg), dim3(256), 0, st, (const uint64_t *)m.p_out, np, (uint64_t)row_bytes, m.start);
		index_scan(m.start, np, m.tiles, m.before, &w->rows, st);
		HD_CHECK(hipGetLastError());
		HD_CHECK(hipMemcpyAsync(&nrows, &w->rows, 8, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
		if (own) {
			if (own->reserve(hd::RowTable::bytes(nrows, true)))
				return HD_E_NOMEM;
			const hd::RowTable t(own->p, nrows, true);
			max_rows = (uint32_t)nrows;
			in_off = t.in_off, out_off = t.out_off, in_len = t.in_len, out_size = t.out_size, reach = t.reach;
		}
		const uint32_t ntab = (uint32_t)(nrows < max_rows ? nrows : max_rows);
		hipLaunchKernelGGL(hd::k_blocks_heads, dim3(nwg), dim3(256), 0, st, (const uint64_t *)c.pos, (const uint32_t *)c.used,
				   (const uint32_t *)c.osize, (const uint32_t *)c.mark, (const uint64_t *)c.rank, ncand, npieces,
				   (const uint64_t *)m.p_out, (const uint32_t *)m.start, (const uint64_t *)m.before, nrows, m.h_pos, m.h_out);
		if (ntab) {
			hipLaunchKernelGGL(hd::k_blocks_rows, dim3((ntab + 255) / 256), dim3(256), 0, st, h_pos, h_out, ntab, max_chunk_in,
					   (uint64_t *)in_off, (uint32_t *)in_len, (uint32_t *)out_size, (uint64_t *)out_off, (uint32_t *)reach, &w->first);
			hipLaunchKernelGGL(hd::k_blocks_reach, dim3(nwg), dim3(256), 0, st, (const uint32_t *)c.reach, (const uint32_t *)c.mark,
					   (const uint64_t *)c.rank, ncand, (const uint64_t *)m.p_out, (const uint32_t *)m.start,
					   (const uint64_t *)m.before, h_out, ntab, (uint32_t *)reach);
			// the reach rule, on the rows in the table: the lowest row at fault by either rule in w->first
			hipLaunchKernelGGL(hd::k_carry_check_reach, dim3((ntab + 255) / 256), dim3(256), 0, st, (const uint32_t *)reach,
					   (const uint64_t *)out_off, ntab, 0xffffffffu, &w->first);
		}
	}
	tm.mark(4, st);
	hipLaunchKernelGGL(hd::k_blocks_verdict, dim3(1), dim3(1), 0, st, src, (const uint64_t *)c.pos, (const uint32_t *)c.used,
			   (const int32_t *)c.pstat, (const uint32_t *)c.stop, ncand, npieces, nrows, max_rows, max_chunk_in, payload_end, trl, h_pos,
			   h_out, &w->rows);
	HD_CHECK(hipGetLastError());
	hd::IndexWords h;
	HD_CHECK(hipMemcpyAsync(&h, w, sizeof h, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	tm.add(g_blocks_ms);
	summary->nrows = h.rows;
	summary->npieces = npieces;
	summary->out_bytes = h.out_bytes;
	summary->end_offset = h.end_offset;
	summary->end_bit = h.spare;
	summary->status = (uint32_t)h.status;
	return 0;
}

int hipdeflate_stream_index_blocks_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_rows, uint32_t max_chunk_in,
				       uint32_t row_bytes, void *in_off, void *in_len, void *out_size, void *out_off, void *reach,
				       hipdeflate_block_index_summary *summary, void *stream)
{
	return blocks_index(cur(), strm, nbytes, frame, max_rows, max_chunk_in, row_bytes, in_off, in_len, out_size, out_off, reach, summary,
			    (hipStream_t)stream, nullptr);
}

int hipdeflate_stream_inflate_blocks_dev(const void *strm, uint64_t nbytes, int frame, const void *in_off, const void *in_len,
					 const void *out_size, const void *out_off, const void *reach, uint32_t nrows, void *out,
					 uint64_t out_cap, hipdeflate_stream_summary *summary, void *stream)
{
	const StreamRows t = { (const uint64_t *)in_off, (const uint32_t *)in_len, (const uint64_t *)out_off, (const uint32_t *)out_size,
			       (const uint32_t *)reach };
	return stream_inflate_rows(cur(), strm, nbytes, frame, t, nullptr, true, nrows, out, out_cap, summary, (hipStream_t)stream, true);
}

/* ---- ... and a seek index on either table: the window in front of every row, and ranged reads on it (hd_seek.hpp) ---- */

int hipdeflate_stream_windows_dev(const void *out, uint64_t out_bytes, const void *out_size, const void *out_off, const void *reach,
				  uint32_t nrows, void *win_off, void *win, uint64_t win_cap, void *row_check,
				  hipdeflate_window_summary *summary, void *stream)
{
	Ctx &g = cur();
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	summary->bad_row = nrows;
	if (nrows >= STREAM_MAX_PARTS || (out_bytes && !out) || (win_cap && !win) ||
	    (nrows && (!out_size || !out_off || !reach || !win_off)))
		return HD_E_ARG;
	if (nrows == 0) {                                                            // a stream has its final row
		summary->status = 1;
		summary->bad_row = 0;
		return 0;
	}
	hipStream_t st = (hipStream_t)stream;
	const uint32_t wg = (nrows + 255) / 256;
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_stream.reserve(hd::WindowScratch::bytes(nrows)))
		return HD_E_NOMEM;
	const hd::WindowScratch d(g.d_stream.p, nrows);
	HD_CHECK(hipMemsetD32Async((hipDeviceptr_t)&d.w->v.fault, (int)hd::IDX_NIL, 1, st));
	hipLaunchKernelGGL(hd::k_seek_check_out, dim3(wg), dim3(256), 0, st, (const uint32_t *)out_size, (const uint64_t *)out_off, nrows,
			   out_bytes, &d.w->v.fault);
	hipLaunchKernelGGL(hd::k_carry_check_reach, dim3(wg), dim3(256), 0, st, (const uint32_t *)reach, (const uint64_t *)out_off, nrows,
			   hd::CARRY_WINDOW, &d.w->v.fault);
	HD_CHECK(hipGetLastError());
	uint32_t fault = hd::IDX_NIL;
	HD_CHECK(hipMemcpyAsync(&fault, &d.w->v.fault, 4, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (fault != hd::IDX_NIL) {
		summary->status = 1;
		summary->bad_row = fault;
		return 0;
	}
	uint64_t *woff = (uint64_t *)win_off;
	index_scan((const uint32_t *)reach, nrows, d.tiles, woff, woff + nrows, st);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&summary->win_bytes, woff + nrows, 8, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (summary->win_bytes > win_cap) {
		summary->status = 3;
		return 0;
	}
	if (summary->win_bytes) {
		const uint64_t cap = (uint64_t)hd::compact_device_cus() * hd::COMPACT_WAVES_PER_CU;
		hipLaunchKernelGGL(hd::k_seek_windows, dim3((uint32_t)(nrows < cap ? nrows : cap)), dim3(64), 0, st, (const uint8_t *)out,
				   (const uint64_t *)out_off, (const uint32_t *)reach, (const uint64_t *)woff, nrows, (uint8_t *)win);
	}
	if (row_check)
		hipLaunchKernelGGL(hd::k_carry_crc, dim3(nrows), dim3(64), 0, st, (const CrcTables *)g.d_ct, (const uint8_t *)out,
				   (const uint64_t *)out_off, (const uint32_t *)out_size, nrows, (uint32_t *)row_check);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipStreamSynchronize(st));
	return 0;
}

int hipdeflate_stream_read_ranges_dev(const void *strm, uint64_t nbytes, int frame, int unit, const void *in_off, const void *in_len,
				      const void *out_size, const void *out_off, const void *reach, const void *win_off, const void *win,
				      uint64_t win_bytes, const void *row_check, uint32_t nrows, const void *q_begin, const void *q_end,
				      uint32_t nqueries, void *dst, uint64_t dst_cap, void *dst_off, void *q_len, void *q_status,
				      hipdeflate_range_summary *summary, void *stream)
{
	Ctx &g = cur();
	int r = enter_call(summary, sizeof *summary);
	if (r)
		return r;
	summary->bad_member = nrows;
	if ((unit != HD_ROWS_BYTES && unit != HD_ROWS_BITS) || !stream_frame_ok(frame) || ((uintptr_t)strm & 15) || (nbytes && !strm) ||
	    nrows >= STREAM_MAX_PARTS || nqueries > 0x7fffffffu ||
	    (nrows && (!in_off || !in_len || !out_size || !out_off || !reach || !win_off || (win_bytes && !win))) ||
	    (nqueries && (!q_begin || !q_end || !dst_off || !q_len || !q_status)) || (!dst && dst_cap))
		return HD_E_ARG;
	if (nrows == 0 || nqueries == 0)
		return 0;
	hipStream_t st = (hipStream_t)stream;
	const bool bits = unit == HD_ROWS_BITS;
	const size_t n = nrows, nq = nqueries;
	const uint32_t wg_n = (nrows + 255) / 256, trl = stream_trl(frame);
	std::lock_guard<std::mutex> lk(g.mu_index);
	if (g.d_stream.reserve(hd::SeekTables::bytes(n)) || g.d_range.reserve(hd::RangeTables::bytes(n, nq)))
		return HD_E_NOMEM;
	const hd::SeekTables d(g.d_stream.p, n);
	const hd::RangeTables t(g.d_range.p, n, nq);
	// 1. the table, by the rules of its unit's decode call, and the windows' offsets
	uint32_t hdr = 0, refused = 0;
	if ((r = stream_open(strm, nbytes, frame, d.header, st, &hdr, &refused)))
		return r;
	if (refused || nbytes < (uint64_t)hdr + trl) {
		summary->status = 1;
		return 0;
	}
	if ((r = stream_words_reset(d.w, hd::CHECK_CRC32, st)))
		return r;
	HD_CHECK(hipMemsetAsync(d.ends, 0, 16, st));
	if (bits)
		hipLaunchKernelGGL(hd::k_blocks_check_rows, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)in_off, (const uint32_t *)in_len,
				   (const uint32_t *)out_size, (const uint64_t *)out_off, nrows, (uint64_t)hdr, nbytes - trl, &d.w->v.fault, d.ends);
	else
		hipLaunchKernelGGL(hd::k_stream_check_rows, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)in_off, (const uint32_t *)in_len,
				   (const uint32_t *)out_size, (const uint64_t *)out_off, nrows, (uint64_t)hdr, nbytes - trl, &d.w->v.fault, d.ends);
	hipLaunchKernelGGL(hd::k_carry_check_reach, dim3(wg_n), dim3(256), 0, st, (const uint32_t *)reach, (const uint64_t *)out_off, nrows,
			   hd::CARRY_WINDOW, &d.w->v.fault);
	hipLaunchKernelGGL(hd::k_seek_check_win, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)win_off, (const uint32_t *)reach, nrows,
			   win_bytes, &d.w->v.fault);
	HD_CHECK(hipGetLastError());
	uint32_t fault = hd::IDX_NIL;
	HD_CHECK(hipMemcpyAsync(&fault, &d.w->v.fault, 4, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	if (fault != hd::IDX_NIL) {
		summary->status = 1;
		summary->bad_member = fault;
		return 0;
	}
	// 2. the queries, as hipdeflate_read_ranges_dev resolves them in bytes: lengths, first rows, coverage -> selection, ranks, layout
	hd::RangeWords *w = t.w, h;
	if ((r = range_plan(t, in_off, in_len, out_size, out_off, nrows, HD_RANGE_BYTES, q_begin, q_end, nqueries, dst_off, q_len, q_status, &h,
			    summary, st)))
		return r;
	if (h.out_bytes > dst_cap) {
		summary->status = 3;
		return 0;
	}
	if (h.nselected == 0)                                                    // no query took a byte
		return 0;
	// 3. the selected rows' tables, back to back in the byte scratch
	const uint32_t nsel = (uint32_t)h.nselected;
	if (g.d_range_out.reserve(h.sel_bytes + 16))
		return HD_E_NOMEM;
	uint8_t *scratch = (uint8_t *)g.d_range_out.p;
	const hd::SeekColumns c{ d.c_in_off, d.c_out_off, d.c_win_off, d.c_in_len, d.c_out_size, d.c_reach, d.c_row_check, d.c_row };
	hipLaunchKernelGGL(hd::k_seek_tables, dim3(wg_n), dim3(256), 0, st, (const uint64_t *)in_off, (const uint32_t *)in_len,
			   (const uint32_t *)out_size, (const uint32_t *)reach, (const uint64_t *)win_off, (const uint32_t *)row_check,
			   (const uint32_t *)t.sel, (const uint64_t *)t.rank, (const uint64_t *)t.scratch_off, nrows, c);
	// 4. and 5. group by group: the rows as symbols, then every symbol its byte -- no group needs another, so nothing is read
	// back between them but the group's record
	const uint64_t group_bytes = g_test_carry_group ? g_test_carry_group : HD_CARRY_GROUP_BYTES;
	for (uint32_t r0 = 0; r0 < nsel;) {
		uint64_t gr[4];
		hipLaunchKernelGGL(hd::k_carry_group, dim3(1), dim3(256), 0, st, (const uint64_t *)d.c_out_off, (const uint32_t *)d.c_out_size,
				   (const uint32_t *)d.c_reach, r0, nsel, group_bytes, d.group);
		HD_CHECK(hipGetLastError());
		HD_CHECK(hipMemcpyAsync(gr, d.group, 32, hipMemcpyDeviceToHost, st));
		HD_CHECK(hipStreamSynchronize(st));
		const uint32_t r1 = (uint32_t)gr[0], nr = r1 - r0;
		const uint64_t begin = gr[2], gbytes = gr[3] - gr[2];
		if (gbytes > (uint64_t)1 << 40 || g.d_stream_slots.reserve(hd::MarkerScratch::bytes(gbytes, 0)))
			return HD_E_NOMEM;
		const hd::MarkerScratch m(g.d_stream_slots.p, gbytes, 0);
		const hd::CarryDecodeArgs da{ (const uint8_t *)strm, d.c_in_off, d.c_in_len, d.c_out_size, d.c_out_off, d.c_reach, r0, nr, begin,
					      m.sym, d.out_len, d.status };
		if (bits)
			hipLaunchKernelGGL(hd::k_blocks_decode, dim3(nr), dim3(64), 0, st, hd::BlocksDecodeArgs{ da });
		else
			hipLaunchKernelGGL(hd::k_carry_decode, dim3(nr), dim3(64), 0, st, da);
		const hd::SeekResolveArgs ra{ m.sym, begin, gr[3], d.c_out_off, d.c_out_size, d.c_reach, d.c_win_off, r0, nr, (const uint8_t *)win,
					      scratch };
		const uint64_t npieces = (gr[3] + hd::SEEK_PIECE - 1) / hd::SEEK_PIECE - begin / hd::SEEK_PIECE;
		hipLaunchKernelGGL(hd::k_seek_resolve, dim3((uint32_t)npieces), dim3(64), 0, st, ra);
		hipLaunchKernelGGL(hd::k_carry_verify, dim3((nr + 255) / 256), dim3(256), 0, st, (const int32_t *)d.status,
				   (const uint32_t *)d.out_len, (const uint32_t *)d.c_out_size, r0, nr, &w->bad_row);
		r0 = r1;
	}
	// 6. the rows' bytes against the checks the caller keeps; the first bad rank by the caller's table
	if (row_check) {
		hipLaunchKernelGGL(hd::k_carry_crc, dim3(nsel), dim3(64), 0, st, (const CrcTables *)g.d_ct, (const uint8_t *)scratch,
				   (const uint64_t *)d.c_out_off, (const uint32_t *)d.c_out_size, nsel, d.crc);
		hipLaunchKernelGGL(hd::k_seek_check_crc, dim3((nsel + 255) / 256), dim3(256), 0, st, (const uint32_t *)d.crc,
				   (const uint32_t *)d.c_row_check, nsel, &w->bad_row);
	}
	hipLaunchKernelGGL(hd::k_range_verdict, dim3(1), dim3(1), 0, st, (const uint32_t *)&w->bad_row, (const uint32_t *)d.c_row, nrows,
			   &w->bad_member);
	// 7. every query's run of the scratch -> dst + dst_off[q]
	const uint64_t grid_cap = (uint64_t)hd::compact_device_cus() * hd::COMPACT_WAVES_PER_CU;
	hipLaunchKernelGGL(hd::k_range_gather, dim3((uint32_t)(h.pieces < grid_cap ? h.pieces : grid_cap)), dim3(64), 0, st,
			   (const uint8_t *)scratch, (const uint64_t *)t.scratch_off, (const uint64_t *)out_off, (const uint32_t *)t.q_first,
			   (const uint64_t *)t.q_from, (const uint32_t *)q_len, (const uint64_t *)dst_off, (const uint64_t *)t.piece_off,
			   nqueries, h.pieces, (uint8_t *)dst);
	HD_CHECK(hipGetLastError());
	HD_CHECK(hipMemcpyAsync(&h.bad_member, &w->bad_member, 8, hipMemcpyDeviceToHost, st));
	HD_CHECK(hipStreamSynchronize(st));
	summary->bad_member = h.bad_member;
	if (h.bad_member != nrows)
		summary->status = 2;
	return 0;
}

/* ---- host-pointer API ------------------------------------------------------ */

// a host dictionary into device memory (Ctx::d_dict; the caller holds g.mu and has bound the device): what the device calls take
static int stage_dict(Ctx &g, const uint8_t *dict, uint32_t dict_len)
{
	if (!dict_len)
		return 0;
	if (g.d_dict.reserve(dict_len))
		return HD_E_NOMEM;
	HD_CHECK(hipMemcpyAsync(g.d_dict.p, dict, dict_len, hipMemcpyHostToDevice, g.stream));
	return 0;
}

// hipdeflate_batch_deflate, and with a dictionary hipdeflate_batch_deflate_dict (frame: HD_FRAME_RAW)
static int batch_deflate_host(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
			      int level, int frame, uint8_t *out, uint64_t out_stride, uint32_t out_cap,
			      uint32_t *out_len, uint32_t *crc32, int32_t *status, const uint8_t *dict, uint32_t dict_len)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!dict && dict_len)
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	if (!in_off || !in_len || !out || !out_len || (frame & ~HD_FRAME_LATENCY) < HD_FRAME_RAW ||
	    (frame & ~HD_FRAME_LATENCY) > HD_FRAME_GZIP)
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device(g)))
		return r;
	if ((r = stage_dict(g, dict, dict_len)))
		return r;

	// pack the blocks 16-byte aligned into pinned memory (one H2D, aligned fast path)
	size_t in_total = 0, max_len = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		in_total += up16(in_len[i]);
		if (in_len[i] > max_len)
			max_len = in_len[i];
	}
	const uint64_t cap_user = out_stride < out_cap ? out_stride : out_cap;
	// device slot: what the user allows, but never more than any encoding needs
	const size_t need = (size_t)hipdeflate_bound(max_len, level);
	const size_t slot = up16(cap_user < need ? cap_user : need);
	const size_t meta_bytes = hd::EncTable::bytes(nblocks);
	if (g.h_in.reserve(in_total + 16) || g.h_meta.reserve(meta_bytes) || g.d_in.reserve(in_total + 16) ||
	    g.d_meta.reserve(meta_bytes) || g.d_slots.reserve(slot * nblocks + 16))
		return HD_E_NOMEM;
	const hd::EncTable h(g.h_meta.p, nblocks), d(g.d_meta.p, nblocks);
	uint8_t *hin = (uint8_t *)g.h_in.p;
	size_t o = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		h.in_off()[i] = o;
		h.in_len()[i] = in_len[i];
		if (in_len[i])
			memcpy(hin + o, in + in_off[i], in_len[i]);
		o += up16(in_len[i]);
	}
	HD_CHECK(hipMemcpyAsync(g.d_in.p, hin, in_total, hipMemcpyHostToDevice, g.stream));
	HD_CHECK(table_copy(d, h, h.inputs(), hipMemcpyHostToDevice, g.stream));
	r = batch_deflate_dev_impl(g.d_in.p, d.in_off(), d.in_len(), nblocks, level, frame, g.d_slots.p, slot,
				   (uint32_t)(cap_user < slot ? cap_user : slot), d.out_len(), d.crc(), d.status(), g.stream,
				   max_len ? (uint32_t)max_len : 1u, 0, dict_len ? g.d_dict.p : nullptr, dict_len);
	if (r)
		return r;
	// gather on the device so that only the compressed bytes cross PCIe
	if ((r = hipdeflate_scan_sizes_dev(d.out_len(), nblocks, 0, d.dst_off(), d.total(), g.stream)))
		return r;
	if (g.d_packed.reserve(slot * nblocks + 16))
		return HD_E_NOMEM;
	if ((r = hipdeflate_compact_dev(g.d_slots.p, slot, d.out_len(), d.dst_off(), nblocks, g.d_packed.p, g.stream)))
		return r;
	HD_CHECK(table_copy(h, d, h.results(), hipMemcpyDeviceToHost, g.stream));
	uint64_t total = 0;
	HD_CHECK(hipMemcpyAsync(&total, d.total(), 8, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipStreamSynchronize(g.stream));
	if (g.h_out.reserve(total + 16))
		return HD_E_NOMEM;
	HD_CHECK(hipMemcpyAsync(g.h_out.p, g.d_packed.p, total, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipStreamSynchronize(g.stream));
	g.stream_drained(g.stream);
	const uint8_t *hp = (const uint8_t *)g.h_out.p;
	size_t po = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		out_len[i] = h.out_len()[i];
		if (crc32)
			crc32[i] = h.crc()[i];
		if (status)
			status[i] = h.status()[i];
		memcpy(out + (uint64_t)i * out_stride, hp + po, out_len[i]);
		po += out_len[i];
	}
	return 0;
}

int hipdeflate_batch_deflate(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
			     int level, int frame, uint8_t *out, uint64_t out_stride, uint32_t out_cap,
			     uint32_t *out_len, uint32_t *crc32, int32_t *status)
{
	return batch_deflate_host(in, in_off, in_len, nblocks, level, frame, out, out_stride, out_cap, out_len, crc32, status, nullptr, 0);
}

int hipdeflate_batch_deflate_dict(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
				  int level, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t out_stride,
				  uint32_t out_cap, uint32_t *out_len, uint32_t *crc32, int32_t *status)
{
	return batch_deflate_host(in, in_off, in_len, nblocks, level, HD_FRAME_RAW, out, out_stride, out_cap, out_len, crc32, status, dict,
				  dict_len);
}

static int batch_inflate_host(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
			      uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
			      uint32_t *crc32, int32_t *status, uint32_t flags)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (nblocks == 0)
		return 0;
	if (!in_off || !in_len || !out_off || !out_cap || !out_len)
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device()))
		return r;
	size_t in_total = 0, out_total = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		if (in_len[i] >= HD_INFLATE_MAX_IN)
			return HD_E_ARG;
		in_total += up16(in_len[i]);
		out_total += up16(out_cap[i]);
	}
	const size_t meta_bytes = hd::DecTable::bytes(nblocks);
	if (g.h_in.reserve(in_total + 16) || g.h_meta.reserve(meta_bytes) || g.d_in.reserve(in_total + 16) ||
	    g.d_meta.reserve(meta_bytes) || g.d_slots.reserve(out_total + 16) || g.h_out.reserve(out_total + 16))
		return HD_E_NOMEM;
	const hd::DecTable h(g.h_meta.p, nblocks), d(g.d_meta.p, nblocks);
	uint8_t *hin = (uint8_t *)g.h_in.p;
	size_t io = 0, oo = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		h.in_off()[i] = io;
		h.out_off()[i] = oo;
		h.in_len()[i] = in_len[i];
		h.out_cap()[i] = out_cap[i];
		if (in_len[i])
			memcpy(hin + io, in + in_off[i], in_len[i]);
		io += up16(in_len[i]);
		oo += up16(out_cap[i]);
	}
	HD_CHECK(hipMemcpyAsync(g.d_in.p, hin, in_total, hipMemcpyHostToDevice, g.stream));
	HD_CHECK(table_copy(d, h, h.inputs(), hipMemcpyHostToDevice, g.stream));
	if ((r = launch_inflate(inflate_args(g, g.d_in.p, d, nblocks, g.d_slots.p, crc32 != nullptr, flags), g.stream)))
		return r;
	HD_CHECK(table_copy(h, d, h.results_crc(), hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipMemcpyAsync(g.h_out.p, g.d_slots.p, out_total, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipStreamSynchronize(g.stream));
	for (uint32_t i = 0; i < nblocks; i++) {
		out_len[i] = h.out_len()[i];
		if (crc32)
			crc32[i] = h.crc()[i];
		if (status)
			status[i] = h.status()[i];
		if (h.status()[i] == 0 && out_len[i])
			memcpy(out + out_off[i], (const uint8_t *)g.h_out.p + h.out_off()[i], out_len[i]);
	}
	return 0;
}

int hipdeflate_batch_inflate(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
			     uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
			     uint32_t *crc32, int32_t *status)
{
	return batch_inflate_host(in, in_off, in_len, nblocks, out, out_off, out_cap, out_len, crc32, status, 0);
}

int hipdeflate_batch_inflate_flush(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
				   uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
				   uint32_t *crc32, int32_t *status)
{
	return batch_inflate_host(in, in_off, in_len, nblocks, out, out_off, out_cap, out_len, crc32, status, hd::INF_FLUSHED);
}

// the members packed 16-byte aligned into pinned memory and sent over, their table into h_off / h_len (HD_E_ARG: one is too long)
static int stage_members(Ctx &g, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
			 uint64_t *h_off, uint32_t *h_len)
{
	size_t in_total = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		if (in_len[i] >= HD_INFLATE_MAX_IN)
			return HD_E_ARG;
		in_total += up16(in_len[i]);
	}
	if (g.h_in.reserve(in_total + 16) || g.d_in.reserve(in_total + 16))
		return HD_E_NOMEM;
	uint8_t *hin = (uint8_t *)g.h_in.p;
	size_t io = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		h_off[i] = io;
		h_len[i] = in_len[i];
		if (in_len[i])
			memcpy(hin + io, in + in_off[i], in_len[i]);
		io += up16(in_len[i]);
	}
	HD_CHECK(hipMemcpyAsync(g.d_in.p, hin, in_total, hipMemcpyHostToDevice, g.stream));
	return 0;
}

int hipdeflate_batch_inflate_size(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				  uint32_t *out_size, uint32_t *in_used, int32_t *status)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!member_frame_ok(frame) || !out_size || !in_used || !status)
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	if (!in_off || !in_len)
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device()))
		return r;
	// in_off u64 | in_len, out_size, in_used, status u32
	const size_t n = nblocks, meta_bytes = 24 * n;
	if (g.h_meta.reserve(meta_bytes) || g.d_meta.reserve(meta_bytes))
		return HD_E_NOMEM;
	uint64_t *h_off = (uint64_t *)g.h_meta.p, *d_off = (uint64_t *)g.d_meta.p;
	uint32_t *h_len = (uint32_t *)(h_off + n), *d_len = (uint32_t *)(d_off + n);
	if ((r = stage_members(g, in, in_off, in_len, nblocks, h_off, h_len)))
		return r;
	HD_CHECK(hipMemcpyAsync(d_off, h_off, 12 * n, hipMemcpyHostToDevice, g.stream));
	if ((r = hipdeflate_batch_inflate_size_dev(g.d_in.p, d_off, d_len, nblocks, frame, d_len + n, d_len + 2 * n, d_len + 3 * n, g.stream)))
		return r;
	HD_CHECK(hipMemcpyAsync(h_len + n, d_len + n, 12 * n, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipStreamSynchronize(g.stream));
	g.stream_drained(g.stream);
	memcpy(out_size, h_len + n, 4 * n);
	memcpy(in_used, h_len + 2 * n, 4 * n);
	memcpy(status, h_len + 3 * n, 4 * n);
	return 0;
}

// hipdeflate_batch_inflate_framed, and with_dict hipdeflate_batch_inflate_dict
static int batch_inflate_framed_host(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				     uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
				     uint32_t *check, uint32_t *in_used, int32_t *status, bool with_dict, const uint8_t *dict,
				     uint32_t dict_len)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!member_frame_ok(frame) || !out_len || !status)
		return HD_E_ARG;
	if (with_dict && (frame == HD_FRAME_GZIP || (!dict && dict_len)))
		return HD_E_ARG;
	if (nblocks == 0)
		return 0;
	if (!in_off || !in_len || !out_off || !out_cap)
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device()))
		return r;
	if (with_dict && (r = stage_dict(g, dict, dict_len)))
		return r;
	// the decode table, and in_used as one more column behind it
	const size_t n = nblocks, meta_bytes = hd::DecTable::bytes(n) + 4 * n;
	size_t out_total = 0;
	for (uint32_t i = 0; i < nblocks; i++)
		out_total += up16(out_cap[i]);
	if (g.h_meta.reserve(meta_bytes) || g.d_meta.reserve(meta_bytes) || g.d_slots.reserve(out_total + 16) ||
	    g.h_out.reserve(out_total + 16))
		return HD_E_NOMEM;
	const hd::DecTable h(g.h_meta.p, n), d(g.d_meta.p, n);
	uint32_t *h_used = (uint32_t *)((uint8_t *)g.h_meta.p + hd::DecTable::bytes(n));
	uint32_t *d_used = (uint32_t *)((uint8_t *)g.d_meta.p + hd::DecTable::bytes(n));
	if ((r = stage_members(g, in, in_off, in_len, nblocks, h.in_off(), h.in_len())))
		return r;
	size_t oo = 0;
	for (uint32_t i = 0; i < nblocks; i++) {
		h.out_off()[i] = oo;
		h.out_cap()[i] = out_cap[i];
		oo += up16(out_cap[i]);
	}
	HD_CHECK(table_copy(d, h, h.inputs(), hipMemcpyHostToDevice, g.stream));
	r = with_dict ? hipdeflate_batch_inflate_dict_dev(g.d_in.p, d.in_off(), d.in_len(), nblocks, frame, dict_len ? g.d_dict.p : nullptr,
							  dict_len, g.d_slots.p, d.out_off(), d.out_cap(), d.out_len(), d.crc(), d_used,
							  d.status(), g.stream)
		      : hipdeflate_batch_inflate_framed_dev(g.d_in.p, d.in_off(), d.in_len(), nblocks, frame, g.d_slots.p, d.out_off(),
							    d.out_cap(), d.out_len(), d.crc(), d_used, d.status(), g.stream);
	if (r)
		return r;
	HD_CHECK(table_copy(h, d, h.results_crc(), hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipMemcpyAsync(h_used, d_used, 4 * n, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipMemcpyAsync(g.h_out.p, g.d_slots.p, out_total, hipMemcpyDeviceToHost, g.stream));
	HD_CHECK(hipStreamSynchronize(g.stream));
	g.stream_drained(g.stream);
	for (uint32_t i = 0; i < nblocks; i++) {
		out_len[i] = h.out_len()[i];
		status[i] = h.status()[i];
		if (check)
			check[i] = h.crc()[i];
		if (in_used)
			in_used[i] = h_used[i];
		if (status[i] == 0 && out_len[i])
			memcpy(out + out_off[i], (const uint8_t *)g.h_out.p + h.out_off()[i], out_len[i]);
	}
	return 0;
}

int hipdeflate_batch_inflate_framed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				    uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
				    uint32_t *check, uint32_t *in_used, int32_t *status)
{
	return batch_inflate_framed_host(in, in_off, in_len, nblocks, frame, out, out_off, out_cap, out_len, check, in_used, status, false,
					 nullptr, 0);
}

int hipdeflate_batch_inflate_dict(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				  const uint8_t *dict, uint32_t dict_len, uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
				  uint32_t *out_len, uint32_t *check, uint32_t *in_used, int32_t *status)
{
	return batch_inflate_framed_host(in, in_off, in_len, nblocks, frame, out, out_off, out_cap, out_len, check, in_used, status, true,
					 dict, dict_len);
}

/* ---- streaming encoder and decoder (SlotRing above) -------------------------------- */

struct hipdeflate_pipe : SlotRing {
	int level, frame;
	uint32_t block, per_batch;
	size_t slot_stride;
};

hipdeflate_pipe *hipdeflate_pipe_open(int level, int frame, uint32_t block_bytes, uint32_t blocks_per_batch, int depth)
{
	if (ensure() || bind_device())
		return nullptr;
	if (frame < HD_FRAME_RAW || frame > HD_FRAME_GZIP || !block_bytes || (block_bytes & 15) || !blocks_per_batch ||
	    depth < 2 || depth > 16 || (uint64_t)block_bytes * blocks_per_batch > 0xffff0000ull)
		return nullptr;
	hipdeflate_pipe *p = new hipdeflate_pipe;
	p->level = level;
	p->frame = frame;
	p->block = block_bytes;
	p->per_batch = blocks_per_batch;
	// a member never needs more than the stored form + the largest frame
	p->slot_stride = (size_t)hipdeflate_bound(block_bytes, level);
	if (frame == HD_FRAME_BGZF && p->slot_stride > 65536)
		p->slot_stride = 65536;
	if (!p->open(depth)) {
		hipdeflate_pipe_close(p);
		return nullptr;
	}
	return p;
}

hipdeflate_pipe *hipdeflate_pipe_open_on(int index, int level, int frame, uint32_t block_bytes, uint32_t blocks_per_batch,
					 int depth)
{
	if (index < 0 || index >= hipdeflate_device_count())
		return nullptr;
	const OnCtx on(index);
	return hipdeflate_pipe_open(level, frame, block_bytes, blocks_per_batch, depth);
}

uint8_t *hipdeflate_pipe_input(hipdeflate_pipe *p, size_t *cap)
{
	if (!p)
		return nullptr;
	const size_t in_cap = (size_t)p->block * p->per_batch;
	PipeSlot *s = p->fill([&](PipeSlot &s) {
		const size_t meta = hd::EncTable::bytes(p->per_batch), packed = p->slot_stride * p->per_batch + 16;
		return s.h_in.reserve(in_cap) || s.d_in.reserve(in_cap + 16) || s.h_meta.reserve(meta) || s.d_meta.reserve(meta) ||
		       s.d_slots.reserve(packed) || s.d_packed.reserve(packed);
	});
	if (!s)
		return nullptr;
	if (cap)
		*cap = in_cap;
	return (uint8_t *)s->h_in.p;
}

int hipdeflate_pipe_submit(hipdeflate_pipe *p, size_t nbytes)
{
	PipeSlot *sp = p ? p->filling() : nullptr;
	if (!sp || nbytes > (size_t)p->block * p->per_batch)
		return HD_E_ARG;
	PipeSlot &s = *sp;
	const OnCtx on(p->ctx);
	int r = ensure();
	if (r || (r = bind_device()))
		return r;
	s.nbytes = nbytes;
	s.nb = (uint32_t)((nbytes + p->block - 1) / p->block);
	if (s.nb) {
		// block table: offsets i * block (16-byte aligned), the last block may be short
		const hd::EncTable h(s.h_meta.p, s.nb), d(s.d_meta.p, s.nb);
		for (uint32_t i = 0; i < s.nb; i++) {
			h.in_off()[i] = (uint64_t)i * p->block;
			h.in_len()[i] = i + 1 < s.nb ? p->block : (uint32_t)(nbytes - (size_t)i * p->block);
		}
		HD_CHECK(hipMemcpyAsync(s.d_in.p, s.h_in.p, nbytes, hipMemcpyHostToDevice, s.st));
		HD_CHECK(table_copy(d, h, h.inputs(), hipMemcpyHostToDevice, s.st));
		if ((r = batch_deflate_dev_impl(s.d_in.p, d.in_off(), d.in_len(), s.nb, p->level, p->frame, s.d_slots.p, p->slot_stride,
						(uint32_t)p->slot_stride, d.out_len(), d.crc(), d.status(), s.st, p->block)))
			return r;
		if ((r = hipdeflate_scan_sizes_dev(d.out_len(), s.nb, 0, d.dst_off(), d.total(), s.st)))
			return r;
		if ((r = hipdeflate_compact_dev(s.d_slots.p, p->slot_stride, d.out_len(), d.dst_off(), s.nb, s.d_packed.p, s.st)))
			return r;
		// sizes, status and the total come back first; the payload follows in result()
		HD_CHECK(table_copy(h, d, h.results_placed(), hipMemcpyDeviceToHost, s.st));
	}
	p->submitted(s);
	return 0;
}

int hipdeflate_pipe_result(hipdeflate_pipe *p, const uint8_t **data, size_t *nbytes, uint32_t *nblocks)
{
	if (!p || !data || !nbytes)
		return HD_E_ARG;
	PipeSlot *sp = p->next_result();
	if (!sp)
		return HD_E_ARG;
	PipeSlot &s = *sp;
	const OnCtx on(p->ctx);
	int r = ensure();
	if (r || (r = bind_device()))
		return r;
	int bad = 0;
	size_t total = 0;
	if (s.nb) {
		HD_CHECK(hipStreamSynchronize(s.st));
		const hd::EncTable h(s.h_meta.p, s.nb);
		total = (size_t)*h.total();
		for (uint32_t i = 0; i < s.nb; i++)
			bad |= h.status()[i] != 0;
		// the pinned landing buffer follows what the data needs (+ 25 %), not the worst case of the slots
		if (s.h_out.reserve(total + 16))
			return HD_E_NOMEM;
		HD_CHECK(hipMemcpyAsync(s.h_out.p, s.d_packed.p, total, hipMemcpyDeviceToHost, s.st));
		HD_CHECK(hipStreamSynchronize(s.st));
	}
	*data = (const uint8_t *)s.h_out.p;
	*nbytes = total;
	if (nblocks)
		*nblocks = s.nb;
	p->hold(s);
	return bad ? 1 : 0;
}

int hipdeflate_pipe_members(hipdeflate_pipe *p, const uint32_t **out_len, const uint64_t **dst_off, const uint32_t **crc32)
{
	if (!p)
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(p->mu);
	if (p->held < 0)
		return HD_E_ARG;                         // no result is held
	const PipeSlot &s = p->slots[p->held];
	const hd::EncTable h(s.h_meta.p, s.nb);
	const bool none = s.nb == 0;             // an empty batch: the pinned table holds an earlier batch's figures
	if (out_len)
		*out_len = none ? nullptr : h.out_len();
	if (crc32)
		*crc32 = none ? nullptr : h.crc();
	if (dst_off)
		*dst_off = none ? nullptr : h.dst_off();
	return 0;
}

void hipdeflate_pipe_close(hipdeflate_pipe *p)
{
	if (!p)
		return;
	p->close();
	delete p;
}

struct hipdeflate_unpipe : SlotRing {
	uint32_t max_members;
	size_t in_cap, out_cap;
};

hipdeflate_unpipe *hipdeflate_unpipe_open(uint32_t max_members, size_t in_cap, size_t out_cap, int depth)
{
	if (ensure() || bind_device())
		return nullptr;
	if (!max_members || !in_cap || !out_cap || depth < 2 || depth > 16 || in_cap > 0xffff0000ull)
		return nullptr;
	hipdeflate_unpipe *p = new hipdeflate_unpipe;
	p->max_members = max_members;
	p->in_cap = in_cap;
	p->out_cap = out_cap;
	if (!p->open(depth)) {
		hipdeflate_unpipe_close(p);
		return nullptr;
	}
	return p;
}

hipdeflate_unpipe *hipdeflate_unpipe_open_on(int index, uint32_t max_members, size_t in_cap, size_t out_cap, int depth)
{
	if (index < 0 || index >= hipdeflate_device_count())
		return nullptr;
	const OnCtx on(index);
	return hipdeflate_unpipe_open(max_members, in_cap, out_cap, depth);
}

uint8_t *hipdeflate_unpipe_input(hipdeflate_unpipe *p, size_t *cap)
{
	if (!p)
		return nullptr;
	PipeSlot *s = p->fill([&](PipeSlot &s) {
		const size_t meta = hd::DecTable::bytes(p->max_members);
		return s.h_in.reserve(p->in_cap) || s.d_in.reserve(p->in_cap + 16) || s.h_meta.reserve(meta) || s.d_meta.reserve(meta) ||
		       s.d_slots.reserve(p->out_cap + 16) || s.h_out.reserve(p->out_cap + 16);
	});
	if (!s)
		return nullptr;
	if (cap)
		*cap = p->in_cap;
	return (uint8_t *)s->h_in.p;
}

int hipdeflate_unpipe_submit(hipdeflate_unpipe *p, const uint64_t *in_off, const uint32_t *in_len,
			     const uint32_t *out_size, uint32_t nmembers)
{
	if (!p || nmembers > p->max_members || (nmembers && (!in_off || !in_len || !out_size)))
		return HD_E_ARG;
	PipeSlot *sp = p->filling();
	if (!sp)
		return HD_E_ARG;
	PipeSlot &s = *sp;
	const OnCtx on(p->ctx);
	int r = ensure();
	if (r || (r = bind_device()))
		return r;
	const uint32_t n = nmembers;
	const hd::DecTable h(s.h_meta.p, n), d(s.d_meta.p, n);
	size_t in_end = 0, osum = 0;
	for (uint32_t i = 0; i < n; i++) {
		if (in_len[i] >= HD_INFLATE_MAX_IN)
			return HD_E_ARG;
		h.in_off()[i] = in_off[i];
		h.in_len()[i] = in_len[i];
		h.out_off()[i] = osum;
		h.out_cap()[i] = out_size[i];
		osum += out_size[i];
		if (in_off[i] + in_len[i] > in_end)
			in_end = (size_t)(in_off[i] + in_len[i]);
	}
	if (in_end > p->in_cap || osum > p->out_cap)
		return HD_E_ARG;
	s.nb = n;
	s.nbytes = osum;
	if (n) {
		HD_CHECK(hipMemcpyAsync(s.d_in.p, s.h_in.p, in_end, hipMemcpyHostToDevice, s.st));
		HD_CHECK(table_copy(d, h, h.inputs(), hipMemcpyHostToDevice, s.st));
		if ((r = launch_inflate(inflate_args(cur(), s.d_in.p, d, n, s.d_slots.p, false, 0), s.st)))
			return r;
		HD_CHECK(table_copy(h, d, h.results(), hipMemcpyDeviceToHost, s.st));
		if (osum)
			HD_CHECK(hipMemcpyAsync(s.h_out.p, s.d_slots.p, osum, hipMemcpyDeviceToHost, s.st));
	}
	p->submitted(s);
	return 0;
}

int hipdeflate_unpipe_result(hipdeflate_unpipe *p, const uint8_t **data, size_t *nbytes)
{
	if (!p || !data || !nbytes)
		return HD_E_ARG;
	PipeSlot *sp = p->next_result();
	if (!sp)
		return HD_E_ARG;
	PipeSlot &s = *sp;
	const OnCtx on(p->ctx);
	int r = ensure();
	if (r || (r = bind_device()))
		return r;
	int verdict = 0;
	if (s.nb) {
		HD_CHECK(hipStreamSynchronize(s.st));
		const hd::DecTable h(s.h_meta.p, s.nb);
		for (uint32_t i = 0; i < s.nb && !verdict; i++)
			verdict = h.status()[i] ? h.status()[i] : (h.out_len()[i] != h.out_cap()[i] ? HD_INSUFFICIENT_SPACE : 0);
	}
	*data = (const uint8_t *)s.h_out.p;
	*nbytes = s.nbytes;
	p->hold(s);
	return verdict;
}

void hipdeflate_unpipe_close(hipdeflate_unpipe *p)
{
	if (!p)
		return;
	p->close();
	delete p;
}

/* ---- latency contexts: small synchronous batches ------------------------------------
 * Everything a call needs is allocated once: pinned, device-visible memory for the blocks, the members and the
 * tables (the kernels read the input and write the members over PCIe themselves -- no copy engine, no staging
 * copy under a lock), device scratch for the segments, one stream.  run() = a handful of launches + one
 * synchronisation.  Contexts are independent: two of them overlap on the device. */
struct hipdeflate_lat {
	int ctx = 0;                                                    // entry of the device list
	int level = 1, frame = HD_FRAME_BGZF;
	uint32_t max_blocks = 0, in_stride = 0, slot = 0;
	hipStream_t st = nullptr;
	Buf h_in{ nullptr, 0, true }, h_out{ nullptr, 0, true }, h_meta{ nullptr, 0, true };
	Buf d_scratch;
	uint8_t *din = nullptr, *dout = nullptr, *dmeta = nullptr;      // device views of the pinned buffers
	bool latency = true;
	uint32_t seg = 0, S = 0;                                        // segment bytes, segment slots per block (0: no segments)
	// the meta buffer: an EncTable of max_blocks | seg_off u64 [max_blocks * S] | seg_len u32 [max_blocks * S] | the poll word
	size_t meta_seg = 0;                                            // offset of the segment table
	hd::EncTable table() const { return { h_meta.p, max_blocks }; }
	hd::EncTable dev_table() const { return { dmeta, max_blocks }; }
	// completion without hipStreamSynchronize (HIPDEFLATE_LAT_POLL): the run's last kernel stores the run's number here
	size_t flag_off = 0;                                            // ... in the meta buffer (pinned, device-visible)
	Buf d_count;                                                    // the word its workgroups count themselves off on
	uint32_t epoch = 0;
};

hipdeflate_lat *hipdeflate_lat_open(int level, int frame, uint32_t max_blocks, uint32_t max_block_bytes)
{
	if (ensure() || bind_device())
		return nullptr;
	const int fr = frame & ~HD_FRAME_LATENCY;
	if (fr < HD_FRAME_RAW || fr > HD_FRAME_GZIP || !max_blocks || max_blocks > 65536 || !max_block_bytes ||
	    max_block_bytes > (64u << 20))
		return nullptr;
	hipdeflate_lat *c = new hipdeflate_lat;
	c->ctx = t_cur;
	c->level = level;
	c->frame = fr;
	c->latency = (frame & HD_FRAME_LATENCY) != 0;
	c->max_blocks = max_blocks;
	c->in_stride = (uint32_t)up16(max_block_bytes);
	c->slot = (uint32_t)hipdeflate_bound(max_block_bytes, level);
	if (fr == HD_FRAME_BGZF && c->slot > 65536)
		c->slot = 65536;
	const SegRule seg = seg_rule(level, c->latency, c->slot);
	c->seg = seg.bytes;
	c->S = seg.limit ? hd::seg_slots_per_block(c->slot, c->seg) : 0;
	c->meta_seg = up16(hd::EncTable::bytes(max_blocks));
	const size_t meta = c->meta_seg + (size_t)max_blocks * c->S * (sizeof(uint64_t) + sizeof(uint32_t)) + 64;
	c->flag_off = meta - 16;
	// (the workgroup levels' records are sized by the longest block, not by the slot)
	const uint64_t scr = scratch_need(max_blocks, level >= HD_WG_LEVEL ? c->in_stride : c->slot, level, c->latency);
	if (c->h_in.reserve((size_t)max_blocks * c->in_stride) || c->h_out.reserve((size_t)max_blocks * c->slot) ||
	    c->h_meta.reserve(meta) || (scr && c->d_scratch.reserve(scr)) || c->d_count.reserve(16) ||
	    hipMemset(c->d_count.p, 0, 16) != hipSuccess ||
	    hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&c->din, c->h_in.p, 0) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&c->dout, c->h_out.p, 0) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&c->dmeta, c->h_meta.p, 0) != hipSuccess) {
		hipdeflate_lat_close(c);
		return nullptr;
	}
	memset(c->h_meta.p, 0, meta);
	for (uint32_t i = 0; i < max_blocks; i++)
		c->table().in_off()[i] = (uint64_t)i * c->in_stride;
	return c;
}

hipdeflate_lat *hipdeflate_lat_open_on(int index, int level, int frame, uint32_t max_blocks, uint32_t max_block_bytes)
{
	if (index < 0 || index >= hipdeflate_device_count())
		return nullptr;
	const OnCtx on(index);
	return hipdeflate_lat_open(level, frame, max_blocks, max_block_bytes);
}

uint8_t *hipdeflate_lat_input(hipdeflate_lat *c, uint32_t i)
{
	return c && i < c->max_blocks ? (uint8_t *)c->h_in.p + (size_t)i * c->in_stride : nullptr;
}

// the run with the frame, the mode and the room per member chosen by the call (the per-block codecs: a context per
// thread serves hip_deflate and hip_deflate_flush, and falls back to the ordinary form when the caller's room is
// below the latency form's worst case)
static int lat_run_ex(hipdeflate_lat *c, const uint32_t *in_len, uint32_t n, int frame, bool latency, uint32_t out_cap)
{
	if (!c || n > c->max_blocks || (n && !in_len))
		return HD_E_ARG;
	if (!n)
		return 0;
	// (a context may outlive hipdeflate_shutdown(), which frees the shared tables: ensure() brings them back)
	const OnCtx on(c->ctx);
	Ctx &g = cur();
	int r = ensure();
	if (r || (r = bind_device()))
		return r;
	const hd::EncTable d = c->dev_table();
	hd::DeflateArgs a = deflate_args(g, c->din, d.in_off(), d.in_len(), n, c->level, frame, latency, c->dout, c->slot,
					 out_cap < c->slot ? out_cap : c->slot, d.out_len(), d.crc(), d.status(),
					 hd::split_max_block(c->slot, c->slot), c->in_stride);
	if (!latency)
		a.seg_limit = 0;                                         // a context codes in segments in latency mode only
	const uint32_t seg_limit = a.seg_limit;
	uint32_t *h_len = c->table().in_len();
	uint32_t hint = hd::HD_HINT_NO_WHOLE | hd::HD_HINT_NO_SEG;
	uint64_t *h_soff = (uint64_t *)((uint8_t *)c->h_meta.p + c->meta_seg);
	uint32_t *h_slen = (uint32_t *)(h_soff + (size_t)c->max_blocks * c->S);
	for (uint32_t i = 0; i < n; i++) {
		if (in_len[i] > c->in_stride)
			return HD_E_ARG;
		h_len[i] = in_len[i];
		const bool segd = hd::seg_coded(in_len[i], seg_limit, c->seg, frame, c->slot, out_cap < c->slot ? out_cap : c->slot);
		hint &= segd ? ~hd::HD_HINT_NO_SEG : ~hd::HD_HINT_NO_WHOLE;
		// the segment table k_seg_table would make (hd_segment.hpp), straight into device-visible memory
		for (uint32_t k = 0; k < c->S; k++) {
			const uint64_t o = (uint64_t)k * c->seg;
			const uint32_t sl = (segd && o < in_len[i]) ? (in_len[i] - o < c->seg ? (uint32_t)(in_len[i] - o) : c->seg) : 0u;
			h_soff[(size_t)i * c->S + k] = (uint64_t)i * c->in_stride + (sl ? o : 0);
			h_slen[(size_t)i * c->S + k] = sl;
		}
	}
	a.scratch = (uint8_t *)c->d_scratch.p;
	if (seg_limit) {
		a.hint = hint;
		a.host_seg_off = (const uint64_t *)(c->dmeta + c->meta_seg);
		a.host_seg_len = (const uint32_t *)(a.host_seg_off + (size_t)c->max_blocks * c->S);
	}
	// the segmented path's last kernel can report by itself (members of up to 64 segments, at least one segmented block)
	static const bool poll_on = [] { const char *e = getenv("HIPDEFLATE_LAT_POLL"); return e && *e && *e != '0'; }();
	const bool poll = poll_on && seg_limit && c->S <= 64 && !(a.hint & hd::HD_HINT_NO_SEG);
	volatile uint32_t *flag = (volatile uint32_t *)((uint8_t *)c->h_meta.p + c->flag_off);
	if (poll) {
		a.done_flag = (uint32_t *)(c->dmeta + c->flag_off);
		a.done_count = (uint32_t *)c->d_count.p;
		a.done_epoch = ++c->epoch ? c->epoch : ++c->epoch;      // (never 0: the word starts as 0)
	}
	if ((r = launch_deflate(a, c->level, c->st)))
		return r;
	if (poll) {
		// ~100 us of kernels: look at the word; should it not come (a fault), the stream's own wait tells
		const auto t0 = std::chrono::steady_clock::now();
		for (uint32_t spins = 0; __atomic_load_n((const uint32_t *)flag, __ATOMIC_ACQUIRE) != a.done_epoch; spins++) {
			__builtin_ia32_pause();
			if ((spins & 4095) == 4095 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(50)) {
				HD_CHECK(hipStreamSynchronize(c->st));
				break;
			}
		}
		return 0;
	}
	HD_CHECK(hipStreamSynchronize(c->st));
	return 0;
}

int hipdeflate_lat_run(hipdeflate_lat *c, const uint32_t *in_len, uint32_t n)
{
	return c ? lat_run_ex(c, in_len, n, c->frame, c->latency, c->slot) : HD_E_ARG;
}

const uint8_t *hipdeflate_lat_output(hipdeflate_lat *c, uint32_t i, uint32_t *out_len, uint32_t *crc32, int32_t *status)
{
	if (!c || i >= c->max_blocks)
		return nullptr;
	const hd::EncTable h = c->table();
	if (out_len)
		*out_len = h.out_len()[i];
	if (crc32)
		*crc32 = h.crc()[i];
	if (status)
		*status = h.status()[i];
	return (const uint8_t *)c->h_out.p + (size_t)i * c->slot;
}

void hipdeflate_lat_close(hipdeflate_lat *c)
{
	if (!c)
		return;
	if (g_all[c->ctx].ready)
		(void)hipSetDevice(g_all[c->ctx].device);
	if (c->st) {
		(void)hipStreamSynchronize(c->st);
		(void)hipStreamDestroy(c->st);
	}
	c->h_in.release();
	c->h_out.release();
	c->h_meta.release();
	c->d_scratch.release();
	c->d_count.release();
	delete c;
}

/* ---- per-block codecs (zlibutil_code_enc / zlibutil_code_dec) --------------- */

// One block per call from each of the caller's threads (zlibutil_buffer_code as a pthread start routine,
// applet/7bgzf.c:211 -- which creates a THREAD PER BLOCK): a call borrows a latency context (blocks up to 64 KiB) from a
// small pool keyed by level and gives it back, so a short-lived thread reuses the pinned buffers, scratch and stream of
// the one before it -- no hipHostMalloc / hipFree per block, no HIP call from a thread-exit destructor, no global
// lock around the coding itself: ~90 us per 0xff00-byte block and thread, all threads at once.  hipdeflate_shutdown()
// closes the pooled contexts.
constexpr uint32_t CODEC_BLOCK = 0x10000;

static hipdeflate_lat *codec_acquire(int level)
{
	const int k = level < 0 ? 0 : level >= CODEC_LEVELS ? CODEC_LEVELS - 1 : level;
	{
		std::lock_guard<std::mutex> lk(g_codec_mu);
		std::vector<hipdeflate_lat *> &f = g_codec_free[k];
		if (!f.empty()) {
			hipdeflate_lat *c = f.back();
			f.pop_back();
			return c;
		}
	}
	// a new context: the per-block codecs' contexts are spread over the device list
	static unsigned rr = 0;
	const int ndev = hipdeflate_device_count();
	const unsigned turn = __atomic_fetch_add(&rr, 1u, __ATOMIC_RELAXED);
	return hipdeflate_lat_open_on(ndev > 0 ? (int)(turn % (unsigned)ndev) : 0, level, HD_FRAME_RAW | HD_FRAME_LATENCY, 1, CODEC_BLOCK);
}

static void codec_release(hipdeflate_lat *c, int level)
{
	const int k = level < 0 ? 0 : level >= CODEC_LEVELS ? CODEC_LEVELS - 1 : level;
	{
		std::lock_guard<std::mutex> lk(g_codec_mu);
		if (g_codec_free[k].size() < CODEC_POOL_MAX) {
			g_codec_free[k].push_back(c);
			return;
		}
	}
	hipdeflate_lat_close(c);
}

extern "C" int hd_codec_batch(unsigned char *dest, size_t *destLen, const unsigned char *src, size_t slen, int level, int flush);
static bool codec_batching()
{
	static const bool on = [] {
		const char *e = getenv("HIPDEFLATE_CODEC_BATCH");
		return !(e && *e == '0');
	}();
	return on;
}

// The room the latency form of one block needs at levels 1 .. HD_WG_LEVEL-1, where a block longer than a segment is cut into
// segments (several wavefronts for the block): their worst case.  0 where nothing is cut: level 0, a block within one
// segment, and the workgroup levels (one stream in either mode, "latency" only picks the kernels that write it)
static uint64_t lat_segments_need(int level, size_t sourceLen, int frame)
{
	return level >= 1 && level < HD_WG_LEVEL && sourceLen > HD_LAT_SEG_BYTES(level)
		       ? HD_SEGN_WORST((uint64_t)sourceLen, HD_LAT_SEG_BYTES(level), frame == HD_FRAME_RAW_FLUSH) : 0;
}

static int deflate_one(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level,
		       int frame)
{
	if (!dest || !destLen || (!source && sourceLen) || sourceLen > 0xffffffffu - 65536u)
		return HD_E_ARG;
	// Concurrent callers -- the reference creates a thread per block, -@N at once (applet/7bgzf.c:211) -- share launches: the
	// hook's micro-batcher with an engine per (level, frame) (bgzf_hook.c hd_codec_batch).  For a block whose room covers
	// the latency form's worst case AND the stored form the bytes do not depend on the room (what the reference's 1.5 x
	// allocation always gives), so callers with different rooms can sit in one batch; everything else takes its own context
	// below.  HIPDEFLATE_CODEC_BATCH=0 turns it off (A/B).
	if (sourceLen && sourceLen <= CODEC_BLOCK && level >= 0 && level <= 9 && codec_batching() && ensure() == 0) {
		const bool fl = frame == HD_FRAME_RAW_FLUSH;
		const uint64_t need_st = HD_STORED_SIZE((uint64_t)sourceLen) + (fl ? 5u : 0u) + 8u;
		if (*destLen >= lat_segments_need(level, sourceLen, frame) && *destLen >= need_st) {
			const int r = hd_codec_batch(dest, destLen, source, sourceLen, level, fl ? 1 : 0);
			if (r == 0 || r == 1)
				return r;                                /* (-1 / -2: not for a batch, or its engine is down) */
		}
	}
	if (sourceLen <= CODEC_BLOCK && ensure() == 0) {
		if (hipdeflate_lat *c = codec_acquire(level)) {
			const size_t cap = *destLen > c->slot ? c->slot : *destLen;
			// latency form only when the room covers its worst case AND the context has a slot for every segment
			const uint64_t need = lat_segments_need(level, sourceLen, frame);
			const bool latency = level >= HD_WG_LEVEL ||
					     (need && cap >= need && HD_SEGN_COUNT((uint32_t)sourceLen, HD_LAT_SEG_BYTES(level)) <= c->S);
			if (sourceLen)
				memcpy(hipdeflate_lat_input(c, 0), source, sourceLen);
			const uint32_t len = (uint32_t)sourceLen;
			int r = lat_run_ex(c, &len, 1, frame, latency, (uint32_t)cap);
			uint32_t olen = 0;
			int32_t st = 0;
			if (!r) {
				const uint8_t *m = hipdeflate_lat_output(c, 0, &olen, nullptr, &st);
				if (st || olen > *destLen)
					r = 1; /* !Z_OK, as libdeflate_deflate (lib/zlibutil.c:189) */
				else
					memcpy(dest, m, olen);
			}
			codec_release(c, level);
			if (!r)
				*destLen = olen;
			return r;
		}
	}
	uint64_t off = 0;
	uint32_t len = (uint32_t)sourceLen, olen = 0;
	int32_t st = 0;
	const size_t cap = *destLen > 0xfffffff0u ? 0xfffffff0u : *destLen;
	// One block per call: latency mode (several wavefronts for the block) whenever the room covers its worst case;
	// the ordinary form otherwise, so that -- as libdeflate_deflate -- the call succeeds whenever the stored form fits
	const uint64_t need = lat_segments_need(level, sourceLen, frame);
	if (level >= HD_WG_LEVEL || (need && cap >= need))
		frame |= HD_FRAME_LATENCY;
	// the slot stride handed to the batch call only needs to cover `cap`
	int r = hipdeflate_batch_deflate(source, &off, &len, 1, level, frame, dest, up16(cap) ? up16(cap) : 16,
					 (uint32_t)cap, &olen, nullptr, &st);
	if (r)
		return r;
	if (st)
		return 1; /* !Z_OK, as libdeflate_deflate (lib/zlibutil.c:189) */
	*destLen = olen;
	return 0;
}

int hip_deflate(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level)
{
	return deflate_one(dest, destLen, source, sourceLen, level, HD_FRAME_RAW);
}

int hip_deflate_flush(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level)
{
	return deflate_one(dest, destLen, source, sourceLen, level, HD_FRAME_RAW_FLUSH);
}

/* ---- per-block decoder: hip_inflate / hip_inflate_flush -----------------------------------------------------------
 * The role of zlibutil_auto_inflate (lib/zlibutil.c:82-93 -> libdeflate_inflate :194-204) as the reference calls it: a
 * THREAD PER BLOCK, -@N of them at once (applet/7bgzf.c:330-345).  One stream is one wavefront's serial work, so what a
 * GPU can give such callers is all of them at once: concurrent calls are coalesced into one launch of the latency kernel
 * (k_inflate_lat: the whole window in LDS) over a batch's pinned, device-visible memory -- every caller copies its own
 * stream in and its own output out with no lock held, the kernel reads and writes that memory itself (no copy engine),
 * the first caller of a batch leads it (closes it once every caller that is inside and not already on the device has
 * joined, launches, waits), the others sleep on the batch's state word.  No process-wide lock around the decoding:
 * HD_CB_CTX batches can be collecting / running side by side, spread over the device list.  A stream or an output
 * larger than a batch's arena goes alone through the host-buffer batch call.  The batching is hd_call_batch.c's, under
 * its decompress policy; this is its client: what a batch owns, what it admits, its launch. */
constexpr uint32_t INFB_SLOTS = 64;                           // streams per batch
constexpr size_t INFB_IN_ARENA = (size_t)5 << 20;             // 64 x (64 KiB + the stored form's overhead) and room to spare
constexpr size_t INFB_OUT_ARENA = (size_t)4 << 20;            // 64 x 64 KiB

struct InfBatch {                                             // what batch context k owns
	int ctx = -1;                                             // entry of the device list
	hipStream_t st = nullptr;
	Buf h_in{ nullptr, 0, true }, h_out{ nullptr, 0, true }, h_meta{ nullptr, 0, true };
	uint8_t *din = nullptr, *dout = nullptr, *dmeta = nullptr;   // device views of the pinned buffers
	size_t in_used = 0, out_used = 0;
	uint32_t flags = 0;
	hd::DecTable table() const { return { h_meta.p, INFB_SLOTS }; }       // pinned, device-visible
	hd::DecTable dev_table() const { return { dmeta, INFB_SLOTS }; }
};
InfBatch g_infb[HD_CB_CTX];

struct InfCall {                                              // what a caller asks of its batch
	size_t sourceLen, ocap, in_need, out_need;
	uint32_t flags;
};

// a batch context's memory and stream
static int inf_open(hd_cb *, int k)
{
	InfBatch &b = g_infb[k];
	static const bool env_once = [] {
		if (const char *w = getenv("HIPDEFLATE_INFLATE_WINDOW_US"))
			hd_cb_inflate.window_ns = atol(w) * 1000;
		if (const char *w = getenv("HIPDEFLATE_INFLATE_LINGER_US"))
			hd_cb_inflate.linger_ns = atol(w) * 1000;
		if (const char *w = getenv("HIPDEFLATE_INFLATE_INFLIGHT"))
			if (atoi(w) >= 1)
				hd_cb_inflate.max_inflight = atoi(w);
		return true;
	}();
	(void)env_once;
	const int ndev = hipdeflate_device_count();
	b.ctx = ndev > 0 ? k % ndev : 0;
	const OnCtx on(b.ctx);
	if (ensure() || bind_device())
		return HD_E_NODEVICE;
	if (b.h_in.reserve(INFB_IN_ARENA + 64) || b.h_out.reserve(INFB_OUT_ARENA + 64) || b.h_meta.reserve(hd::DecTable::bytes(INFB_SLOTS)) ||
	    hipStreamCreateWithFlags(&b.st, hipStreamNonBlocking) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&b.din, b.h_in.p, 0) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&b.dout, b.h_out.p, 0) != hipSuccess ||
	    hipHostGetDevicePointer((void **)&b.dmeta, b.h_meta.p, 0) != hipSuccess) {
		b.h_in.release();
		b.h_out.release();
		b.h_meta.release();
		if (b.st)
			(void)hipStreamDestroy(b.st);
		b.st = nullptr;
		return HD_E_NOMEM;
	}
	return 0;
}

// a batch holds streams of one `flags` value, as many as its arenas have room for
static int inf_admit(hd_cb *, int k, int idx, const void *req)
{
	InfBatch &b = g_infb[k];
	const InfCall &c = *(const InfCall *)req;
	if (idx == 0) {
		b.in_used = b.out_used = 0;
		b.flags = c.flags;
	} else if (b.flags != c.flags || b.in_used + c.in_need > INFB_IN_ARENA || b.out_used + c.out_need > INFB_OUT_ARENA) {
		return 0;
	}
	const hd::DecTable t = b.table();
	t.in_off()[idx] = b.in_used;
	t.out_off()[idx] = b.out_used;
	t.in_len()[idx] = (uint32_t)c.sourceLen;
	t.out_cap()[idx] = (uint32_t)c.ocap;
	b.in_used += c.in_need;
	b.out_used += c.out_need;
	return 1;
}

static int inf_run(hd_cb *, int k, int n)
{
	InfBatch &b = g_infb[k];
	const OnCtx on(b.ctx);
	int rc;
	if ((rc = ensure()) || (rc = bind_device()))
		return rc;
	const hd::InflateArgs a = inflate_args(cur(), b.din, b.dev_table(), (uint32_t)n, b.dout, false, b.flags);
	hipLaunchKernelGGL(hd::k_inflate_lat, dim3((uint32_t)n), dim3(hd::INF_LAT_THREADS), 0, b.st, a);      // (four wavefronts per stream: hd_inflate_lat.hpp)
	if (hipGetLastError() != hipSuccess || hipStreamSynchronize(b.st) != hipSuccess) {
		fprintf(stderr, "hipdeflate: hip_inflate: the latency kernel did not run\n");
		return HD_E_NODEVICE;
	}
	return 0;
}

static void inf_close(hd_cb *, int k)
{
	InfBatch &b = g_infb[k];
	if (g_all[b.ctx].ready)
		(void)hipSetDevice(g_all[b.ctx].device);
	(void)hipStreamSynchronize(b.st);
	(void)hipStreamDestroy(b.st);
	b.st = nullptr;
	b.h_in.release();
	b.h_out.release();
	b.h_meta.release();
}

static const hd_cb_client g_infb_client = { inf_open, inf_admit, inf_run, inf_close };
static hd_cb g_infb_eng = HD_CB_INIT(&g_infb_client, &hd_cb_inflate_policy, nullptr, INFB_SLOTS);

static void infb_drain()                                      // hipdeflate_shutdown(): idle batch contexts are closed, a failure is forgotten
{
	hd_cb_drain(&g_infb_eng);
}

static int inflate_alone(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, uint32_t flags)
{
	uint64_t ioff = 0, ooff = 0;
	uint32_t ilen = (uint32_t)sourceLen, olen = 0;
	uint32_t ocap = *destLen > 0xfffffff0u ? 0xfffffff0u : (uint32_t)*destLen;
	int32_t st = 0;
	int r = batch_inflate_host(source, &ioff, &ilen, 1, dest, &ooff, &ocap, &olen, nullptr, &st, flags);
	if (r)
		return r;
	if (st)
		return st;
	*destLen = olen;
	return 0;
}

static int inflate_one(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, uint32_t flags)
{
	if (!dest || !destLen || (!source && sourceLen) || sourceLen >= HD_INFLATE_MAX_IN)
		return HD_E_ARG;
	const size_t ocap = *destLen > 0xfffffff0u ? 0xfffffff0u : *destLen;
	const size_t in_need = up16(sourceLen + 4), out_need = up16(ocap);       // (+4: the kernel reads whole dwords)
	if (in_need > INFB_IN_ARENA / 4 || out_need > INFB_OUT_ARENA / 4)
		return inflate_alone(dest, destLen, source, sourceLen, flags);

	const InfCall c = { sourceLen, ocap, in_need, out_need, flags };
	hd_cb_seat s;
	// HD_E_NOMEM (the batch contexts' pinned memory): this caller and later ones go alone, until hipdeflate_shutdown()
	if (const int f = hd_cb_join(&g_infb_eng, &c, &s))
		return f == HD_E_NOMEM ? inflate_alone(dest, destLen, source, sourceLen, flags) : f;
	const InfBatch &b = g_infb[s.k];
	const hd::DecTable t = b.table();
	if (sourceLen)
		memcpy((uint8_t *)b.h_in.p + t.in_off()[s.idx], source, sourceLen);      /* own stream, no lock held */
	int ret = hd_cb_wait(&g_infb_eng, &s);
	if (!ret && !(ret = t.status()[s.idx])) {
		const uint32_t olen = t.out_len()[s.idx];
		if (olen)
			memcpy(dest, (const uint8_t *)b.h_out.p + t.out_off()[s.idx], olen);   /* own output, no lock held */
		*destLen = olen;
	}
	hd_cb_leave(&g_infb_eng, &s);
	return ret;
}

void hipdeflate_test_beside(int keep, uint32_t sub_cap)
{
	g_test_beside_keep = keep < 0 ? 0u : (uint32_t)keep > hd::BESIDE_KEEP_MAX ? hd::BESIDE_KEEP_MAX : (uint32_t)keep;
	hd::wg_sub_test() = sub_cap;
}

uint32_t hipdeflate_test_compact_grid(void)
{
	Ctx &g = cur();
	std::lock_guard<std::mutex> lk(g.mu_enc);
	return g.compact_grid;
}

#ifdef HD_EMIT_STATS
int hipdeflate_test_emit_stats(uint64_t *out16)   // [0,8) phases of the emit kernel, [8,16) of build_code for the litlen alphabet
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(hd::g_emit_stats), 128));
	return 0;
}
int hipdeflate_test_emit_stats32(uint64_t *out32)   // ... and [16,32): k_emit_wg's block builder
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out32, HIP_SYMBOL(hd::g_emit_stats), 256));
	return 0;
}
#endif

#ifdef HD_CLOCK_STAMPS
// diagnostic build: sums of cycles from wave start to the marks of the level-1 / parse kernel (read and cleared)
int hipdeflate_test_clock_marks(uint64_t *out16)
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(hd::g_clk_mark), 128));
	static const uint64_t zero[16] = { 0 };
	HD_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(hd::g_clk_mark), zero, 128));
	return 0;
}
// diagnostic build: per kernel { shader cycles, 100 MHz ticks, waves, - } summed over the waves since the last call
int hipdeflate_test_clock(uint64_t *out16)
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out16, HIP_SYMBOL(hd::g_clk), 128));
	static const uint64_t zero[16] = { 0 };
	HD_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(hd::g_clk), zero, 128));
	return 0;
}
#endif

#ifdef HD_INFLATE_STATS
int hipdeflate_test_inflate_stats(uint64_t *out8)
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(hd::g_inf_stats), 64));
	// slots 6, 7 are reused for nothing: the cycle counters follow behind when the caller left room for 16 words
	return 0;
}
int hipdeflate_test_inflate_stats2(uint64_t *out8)
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(hd::g_inf_stats2), 64));
	return 0;
}
int hipdeflate_test_inflate_cycles(uint64_t *out8)
{
	HD_CHECK(hipDeviceSynchronize());
	HD_CHECK(hipMemcpyFromSymbol(out8, HIP_SYMBOL(hd::g_inf_cycles), 64));
	return 0;
}
#endif

int hip_inflate(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen)
{
	return inflate_one(dest, destLen, source, sourceLen, 0);
}

int hip_inflate_flush(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen)
{
	return inflate_one(dest, destLen, source, sourceLen, hd::INF_FLUSHED);
}

// hip_deflate_stream and, with every chunk primed by the bytes in front of it (carry), hip_deflate_stream_carry: stage, code, fetch
static int deflate_stream_host(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level, int frame,
			       uint32_t chunk_bytes, bool carry)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!destLen || (*destLen && !dest) || (sourceLen && !source) || !stream_frame_ok(frame) || !stream_chunk_ok(chunk_bytes))
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device(g)))
		return r;
	const uint64_t bound = hipdeflate_stream_bound(sourceLen, chunk_bytes, level, frame);
	const uint64_t cap = *destLen < bound ? *destLen : bound;
	if (g.d_in.reserve(up16(sourceLen) + 16) || g.d_packed.reserve(up16(cap) + 16))
		return HD_E_NOMEM;
	if (sourceLen)
		HD_CHECK(hipMemcpyAsync(g.d_in.p, source, sourceLen, hipMemcpyHostToDevice, g.stream));
	hipdeflate_stream_summary s;
	if ((r = stream_deflate_impl(g.d_in.p, sourceLen, chunk_bytes, level, frame, g.d_packed.p, cap, nullptr, &s, g.stream,
				     carry ? HD_WG_WINDOW : 0u)))
		return r;
	g.stream_drained(g.stream);
	if (s.status)
		return 1;
	HD_CHECK(hipMemcpy(dest, g.d_packed.p, s.out_bytes, hipMemcpyDeviceToHost));
	*destLen = s.out_bytes;
	return 0;
}

int hip_deflate_stream(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level, int frame,
		       uint32_t chunk_bytes)
{
	return deflate_stream_host(dest, destLen, source, sourceLen, level, frame, chunk_bytes, false);
}

int hip_deflate_stream_carry(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int level, int frame,
			     uint32_t chunk_bytes)
{
	return deflate_stream_host(dest, destLen, source, sourceLen, level, frame, chunk_bytes, true);
}

// hip_inflate_stream and, for a stream whose flushes carry the window (carry), hip_inflate_stream_carry: stage, index,
// decode.  The row table stays on the device, in d_meta, as large as the stream needs
// blocks: hip_inflate_stream_blocks -- the block index and its bit rows (hd_blocks.hpp), with the carry decode's table
static int inflate_stream_host(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame,
			       size_t *in_used, bool carry, bool blocks = false)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!destLen || (*destLen && !dest) || (sourceLen && !source) || !stream_frame_ok(frame))
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device(g)))
		return r;
	if (g.d_in.reserve(up16(sourceLen) + 16))
		return HD_E_NOMEM;
	if (sourceLen)
		HD_CHECK(hipMemcpyAsync(g.d_in.p, source, sourceLen, hipMemcpyHostToDevice, g.stream));
	hipdeflate_stream_index_summary xs;
	if (blocks) {
		hipdeflate_block_index_summary bs;
		// a piece of HD_BLOCK_PIECE_IN bytes at the most first: that bounds what a false candidate can cost.  Status 1 may then
		// be the bound's doing (a long stored span, a writer of larger blocks): only then the unbounded index decides
		if ((r = blocks_index(g, g.d_in.p, sourceLen, frame, 0, HD_BLOCK_PIECE_IN, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &bs, g.stream,
				      &g.d_meta)))
			return r;
		if (bs.status == 1 && sourceLen > HD_BLOCK_PIECE_IN &&
		    (r = blocks_index(g, g.d_in.p, sourceLen, frame, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &bs, g.stream, &g.d_meta)))
			return r;
		xs = { bs.nrows, bs.out_bytes, bs.end_offset, bs.ncandidates, bs.hdr_bytes, bs.status };
	} else if ((r = stream_index(g, g.d_in.p, sourceLen, frame, 0, 0, nullptr, nullptr, nullptr, nullptr, &xs, g.stream, &g.d_meta, carry))) {
		return r;
	}
	g.stream_drained(g.stream);
	if (in_used)
		*in_used = xs.end_offset;
	if (xs.status)
		return 1;
	if (xs.out_bytes > *destLen) {
		*destLen = xs.out_bytes;
		return 3;
	}
	if (g.d_packed.reserve(up16(xs.out_bytes) + 16))
		return HD_E_NOMEM;
	const hd::RowTable t(g.d_meta.p, xs.nchunks, carry);         // (status 0: the chain's rows, which the table's layout goes by)
	hipdeflate_stream_summary s;
	if ((r = stream_inflate_rows(g, g.d_in.p, xs.end_offset, frame, { t.in_off, t.in_len, t.out_off, t.out_size, t.reach }, nullptr, carry,
				     (uint32_t)xs.nchunks, g.d_packed.p, xs.out_bytes, &s, g.stream, blocks)))
		return r;
	if (s.status)
		return 1;
	if (xs.out_bytes)
		HD_CHECK(hipMemcpy(dest, g.d_packed.p, xs.out_bytes, hipMemcpyDeviceToHost));
	*destLen = xs.out_bytes;
	return 0;
}

int hip_inflate_stream(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame, size_t *in_used)
{
	return inflate_stream_host(dest, destLen, source, sourceLen, frame, in_used, false);
}

int hip_inflate_stream_carry(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame, size_t *in_used)
{
	return inflate_stream_host(dest, destLen, source, sourceLen, frame, in_used, true);
}

int hip_inflate_stream_blocks(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame, size_t *in_used)
{
	return inflate_stream_host(dest, destLen, source, sourceLen, frame, in_used, true, true);
}

// stage, index (the sizing call, then on a table of that size in d_meta), inflate into d_packed, verify
int hip_inflate_members(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, size_t *in_used)
{
	Ctx &g = cur();
	int r = ensure();
	if (r)
		return r;
	if (!destLen || (*destLen && !dest) || (sourceLen && !source))
		return HD_E_ARG;
	std::lock_guard<std::mutex> lk(g.mu);
	if ((r = bind_device(g)))
		return r;
	if (g.d_in.reserve(up16(sourceLen) + 16))
		return HD_E_NOMEM;
	if (sourceLen)
		HD_CHECK(hipMemcpyAsync(g.d_in.p, source, sourceLen, hipMemcpyHostToDevice, g.stream));
	hipdeflate_member_any_summary ms;
	if ((r = hipdeflate_index_members_any_dev(g.d_in.p, sourceLen, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, &ms, g.stream)))
		return r;
	if (ms.status == 3) {
		if (ms.nmembers > 0x7fffffffu || g.d_meta.reserve(hd::MemberTables::bytes((size_t)ms.nmembers)))
			return HD_E_NOMEM;
		const hd::MemberTables t(g.d_meta.p, (size_t)ms.nmembers);
		if ((r = hipdeflate_index_members_any_dev(g.d_in.p, sourceLen, 0, (uint32_t)ms.nmembers, 0, t.in_off, t.in_len, t.out_size, t.out_off,
							  t.crc_want, &ms, g.stream)))
			return r;
	}
	g.stream_drained(g.stream);
	if (in_used)
		*in_used = ms.end_offset;
	if (ms.status)
		return 1;
	if (ms.out_bytes > *destLen) {
		*destLen = ms.out_bytes;
		return 3;
	}
	const uint32_t n = (uint32_t)ms.nmembers;
	if (n) {
		if (g.d_packed.reserve(up16(ms.out_bytes) + 16))
			return HD_E_NOMEM;
		const hd::MemberTables t(g.d_meta.p, n);
		if ((r = launch_inflate({ (const uint8_t *)g.d_in.p, t.in_off, t.in_len, n, (uint8_t *)g.d_packed.p, t.out_off, t.out_size, t.out_len, t.crc,
					  t.status, g.d_ct, 0 },
					g.stream)))
			return r;
		uint64_t bad = n;
		if ((r = hipdeflate_verify_members_dev(t.status, t.out_len, t.crc, t.out_size, t.crc_want, n, &bad, g.stream)))
			return r;
		if (bad != n)
			return 1;
		if (ms.out_bytes)
			HD_CHECK(hipMemcpy(dest, g.d_packed.p, ms.out_bytes, hipMemcpyDeviceToHost));
	}
	*destLen = ms.out_bytes;
	return 0;
}

} // extern "C"
