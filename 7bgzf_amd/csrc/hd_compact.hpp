// hd_compact.hpp -- size prefix scan + member gather.
//
// Role: the in-order writer of applet/7bgzf.c:223-272 (join threads in order,
// fwrite each member) becomes "exclusive prefix sum of the member sizes, then
// every member copied to its final offset", all on the device.  With several
// GPUs each rank adds its base (the all-gathered totals of the lower ranks,
// SURVEY.md 8(e)) through the `base` argument.  HBM-bound byte copy.
#pragma once
#include "hd_device.hpp"
#include <atomic>

namespace hd {

constexpr uint32_t SCAN_TILE = 2048;     // elements per 256-thread workgroup

// pass 1: per-tile sums
__global__ __launch_bounds__(256) void k_scan_tile_sums(const uint32_t *len, uint32_t n, uint64_t *tile_sum)
{
	__shared__ uint64_t wsum[4];
	const uint32_t t = threadIdx.x, tile = blockIdx.x;
	uint64_t s = 0;
	for (uint32_t i = tile * SCAN_TILE + t; i < n && i < (tile + 1) * SCAN_TILE; i += 256)
		s += len[i];
	for (int o = 32; o > 0; o >>= 1) {
		s += ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)s, o, 64)) |
		     ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(s >> 32), o, 64) << 32);
	}
	if ((t & 63) == 0)
		wsum[t >> 6] = s;
	__syncthreads();
	if (t == 0)
		tile_sum[tile] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// pass 2: one workgroup turns tile sums into exclusive tile offsets (+ base)
__global__ __launch_bounds__(256) void k_scan_tiles(uint64_t *tile_sum, uint32_t ntiles, uint64_t base, uint64_t *total)
{
	__shared__ uint64_t part[256];
	const uint32_t t = threadIdx.x;
	const uint32_t per = (ntiles + 255) / 256;
	uint64_t s = 0;
	for (uint32_t k = 0; k < per; k++) {
		const uint32_t i = t * per + k;
		if (i < ntiles)
			s += tile_sum[i];
	}
	part[t] = s;
	__syncthreads();
	if (t == 0) {
		uint64_t run = base;
		for (uint32_t k = 0; k < 256; k++) {
			const uint64_t v = part[k];
			part[k] = run;
			run += v;
		}
		if (total)
			*total = run - base;
	}
	__syncthreads();
	uint64_t run = part[t];
	for (uint32_t k = 0; k < per; k++) {
		const uint32_t i = t * per + k;
		if (i < ntiles) {
			const uint64_t v = tile_sum[i];
			tile_sum[i] = run;
			run += v;
		}
	}
}

// pass 3: exclusive scan inside each tile.  The intra-tile sums are 64 bits wide like the other two passes:
// a tile of 2048 members of >= 2 MiB each (MiGz -b, the uint32 in_len API) passes 4 GiB.
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t x)
{
	// x < 2^35 per lane (eight u32): split at bit 26, so that both 32-bit DPP scans stay carry-free
	// (64 x 2^26 = 2^32 is never reached, 64 x 2^9 is tiny)
	const uint32_t a = wave_incl_scan((uint32_t)x & 0x3ffffffu);
	const uint64_t b = wave_incl_scan((uint32_t)(x >> 26));
	return (uint64_t)a + (b << 26);
}

__global__ __launch_bounds__(256) void k_scan_finish(const uint32_t *len, uint32_t n, const uint64_t *tile_off, uint64_t *dst_off)
{
	__shared__ uint64_t wtot[4];
	const uint32_t t = threadIdx.x, tile = blockIdx.x, lane = t & 63, w = t >> 6;
	// thread t owns 8 consecutive elements
	const uint32_t i0 = tile * SCAN_TILE + t * 8;
	uint32_t v[8];
	uint64_t s = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		v[k] = i0 + k < n ? len[i0 + k] : 0;
		s += v[k];
	}
	const uint64_t incl = wave_incl_scan64(s);
	if (lane == 63)
		wtot[w] = incl;
	__syncthreads();
	uint64_t run = tile_off[tile] + (incl - s);
	for (uint32_t k = 0; k < w; k++)
		run += wtot[k];
#pragma unroll
	for (int k = 0; k < 8; k++) {
		if (i0 + k < n)
			dst_off[i0 + k] = run;
		run += v[k];
	}
}

// one wavefront copies L bytes from s (16-byte aligned) to d (any alignment), whole destination dwords in the middle
__device__ __forceinline__ void compact_one(const uint8_t *s, uint32_t L, uint8_t *d, uint32_t lane)
{
	// head: bytes until d is dword aligned
	uint32_t head = (uint32_t)((4 - ((uintptr_t)d & 3)) & 3);
	if (head > L)
		head = L;
	if (lane < head)
		d[lane] = s[lane];
	const uint32_t body = (L - head) >> 2;           // whole destination dwords
	const uint32_t *s32 = (const uint32_t *)s;       // source dwords (aligned)
	uint32_t *d32 = (uint32_t *)(d + head);
	for (uint32_t k = lane; k < body; k += 64) {
		// destination dword k = source bytes [head + 4k, head + 4k + 4)
		const uint32_t so = head + 4 * k;
		const uint32_t lo = s32[so >> 2];
		const uint32_t hi = (so & 3) ? s32[(so >> 2) + 1] : 0;
		d32[k] = __builtin_amdgcn_alignbyte(hi, lo, so & 3);
	}
	const uint32_t done = head + 4 * body;
	if (lane < L - done)
		d[done + lane] = s[done + lane];
}

// ---- the gather: 16 bytes per lane and access, several in flight, a persistent grid ---------------------------------
//
// A member's bytes go from its slot (4-byte aligned, any length) to dst + dst_off[i] (any alignment).  The body is whole
// 16-byte lines of the DESTINATION, stored with global_store_dwordx4; their source bytes arrive by 16-byte loads from
// whatever address that makes (gfx950 takes a byte-aligned global_load_dwordx4), so the copy runs no funnel shift and no
// vector ALU beyond its addresses.  A wavefront moves COMPACT_GROUP bytes per trip of its loop: COMPACT_UNROLL loads per
// lane, one wait, COMPACT_UNROLL stores, one back edge.  The ragged ends of a member -- up to 15 bytes in front of the
// first whole line and up to 15 behind the last -- are byte stores of one lane each: two members' wavefronts may share a
// 16-byte line, so no line is ever read, merged and written back.  Exactly the member's bytes are read, none beside them.
// Loads and stores are nontemporal: they pass the CU's L1 by, which the encode kernel running beside the gather uses for
// its own tables (worth 0.1 ms of the encoder's 45).
// The three figures of the kernel, each overridable from the compiler's command line (make EXTRA=-DHD_COMPACT_...=...),
// which is how the rows of DESIGN.md 6d were built from this one source.
#ifndef HD_COMPACT_UNROLL
#define HD_COMPACT_UNROLL 4
#endif
#ifndef HD_COMPACT_NT
#define HD_COMPACT_NT 1
#endif
#ifndef HD_COMPACT_WAVES_PER_CU
#define HD_COMPACT_WAVES_PER_CU 3
#endif
constexpr uint32_t COMPACT_UNROLL = HD_COMPACT_UNROLL;              // 16-byte accesses per lane between two waits
constexpr uint32_t COMPACT_GROUP = 64 * 16 * COMPACT_UNROLL;        // bytes per wavefront and trip of the body loop
constexpr bool COMPACT_NT = HD_COMPACT_NT != 0;                     // nontemporal loads and stores
// The persistent grid, wavefronts per CU.  What the gather takes from an encode kernel beside it grows with the bytes it
// keeps in flight, not with the instructions it issues: 3 x 4 KiB per CU is the least that still copies, alone, as fast
// as one wavefront per member did (DESIGN.md 6d has the sweep).
constexpr uint32_t COMPACT_WAVES_PER_CU = HD_COMPACT_WAVES_PER_CU;
// The small grid, wavefronts per TWO CUs (so that half a wavefront per CU can be written down): what a gather gets that
// the library itself launches while an encode kernel of its own is still running in another stream (hd_api.hip
// compact_beside).  Such a gather has that kernel's whole time to spare and need not be fast, only gentle: throttled
// like this it takes a fraction of what the full grid takes from the encoder (DESIGN.md 6d has the sweep).
#ifndef HD_COMPACT_BESIDE_WAVES_PER_2CU
#define HD_COMPACT_BESIDE_WAVES_PER_2CU 1
#endif
constexpr uint32_t COMPACT_BESIDE_WAVES_PER_2CU = HD_COMPACT_BESIDE_WAVES_PER_2CU;
static_assert(COMPACT_BESIDE_WAVES_PER_2CU >= 1 && COMPACT_BESIDE_WAVES_PER_2CU <= 2 * COMPACT_WAVES_PER_CU, "the small grid is not above the full one");

typedef uint32_t compact_u32x4 __attribute__((ext_vector_type(4)));
typedef compact_u32x4 compact_u32x4_any __attribute__((aligned(1)));   // a source line: wherever the destination's alignment puts it

template <bool NT>
__device__ __forceinline__ compact_u32x4 compact_ld16(const uint8_t *p)
{
	const compact_u32x4_any *q = (const compact_u32x4_any *)p;
	if (NT)
		return __builtin_nontemporal_load(q);
	return *q;
}

template <bool NT>
__device__ __forceinline__ void compact_st16(uint8_t *p, compact_u32x4 v)
{
	compact_u32x4 *q = (compact_u32x4 *)p;
	if (NT)
		__builtin_nontemporal_store(v, q);
	else
		*q = v;
}

template <bool NT, uint32_t U>
__device__ __forceinline__ void compact_wide(const uint8_t *__restrict__ s, uint32_t L, uint8_t *__restrict__ d, uint32_t lane)
{
	uint32_t head = (uint32_t)(0 - (uintptr_t)d) & 15;        // bytes in front of the first whole destination line
	if (head > L)
		head = L;
	const uint32_t lines = (L - head) >> 4;                   // whole destination lines
	const uint32_t done = head + 16 * lines;
	// both ragged ends in one byte access: lanes 0..15 the head, lanes 16..31 the tail; requested ahead of the body
	const uint32_t eo = lane < 16 ? lane : done + lane - 16;
	const bool edge = lane < 16 ? lane < head : lane < 32 && lane - 16 < L - done;
	uint8_t eb = 0;
	if (edge)
		eb = s[eo];
	const uint8_t *sb = s + head + 16 * lane;
	uint8_t *db = d + head + 16 * lane;
	uint32_t k = 0;                                           // the trip's first line (uniform)
	for (; k + 64 * U <= lines; k += 64 * U) {
		compact_u32x4 v[U];
#pragma unroll
		for (uint32_t j = 0; j < U; j++)
			v[j] = compact_ld16<NT>(sb + 16 * (k + 64 * j));
#pragma unroll
		for (uint32_t j = 0; j < U; j++)
			compact_st16<NT>(db + 16 * (k + 64 * j), v[j]);
	}
	// the lines left, fewer than a trip's: the same group once more, a lane past the end loading the last line again
	// (no branch round a load) and storing nothing
	if (k < lines) {
		compact_u32x4 v[U];
		uint32_t q[U];
#pragma unroll
		for (uint32_t j = 0; j < U; j++) {
			q[j] = k + 64 * j + lane;
			v[j] = compact_ld16<NT>(s + head + 16 * (uint64_t)(q[j] < lines ? q[j] : lines - 1));
		}
#pragma unroll
		for (uint32_t j = 0; j < U; j++)
			if (q[j] < lines)
				compact_st16<NT>(d + head + 16 * (uint64_t)q[j], v[j]);
	}
	if (edge)
		d[eo] = eb;
}

// slots + i*stride (4-byte aligned) -> dst + dst_off[i].  A grid of at least n wavefronts is one wavefront per member;
// a smaller one is persistent, wavefront w taking members w, w + grid, ...; the next member's length and offset are
// requested before the current member is copied.
__global__ __launch_bounds__(64) void k_compact(const uint8_t *__restrict__ slots, uint64_t stride, const uint32_t *__restrict__ len,
						const uint64_t *__restrict__ dst_off, uint32_t n, uint8_t *__restrict__ dst)
{
	const uint32_t lane = threadIdx.x, step = gridDim.x;
	uint32_t i = blockIdx.x;
	if (i >= n)
		return;
	uint32_t L = len[i];
	uint64_t o = dst_off[i];
	for (;;) {
		const uint32_t nx = i + step;
		const bool more = nx < n && nx > i;
		const uint32_t nc = more ? nx : i;                // (no branch round the two scalar loads)
		const uint32_t Ln = len[nc];
		const uint64_t on = dst_off[nc];
		compact_wide<COMPACT_NT, COMPACT_UNROLL>(slots + (uint64_t)i * stride, L, dst + o, lane);
		if (!more)
			break;
		i = nx;
		L = Ln;
		o = on;
	}
}

// compute units of the calling thread's device (the persistent grid's measure), asked once per device
inline uint32_t compact_device_cus()
{
	static std::atomic<uint32_t> cus[64];
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)
		return 256;
	uint32_t c = cus[dev].load(std::memory_order_relaxed);
	if (!c) {
		int v = 0;
		if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
			v = 256;
		cus[dev].store(c = (uint32_t)v, std::memory_order_relaxed);
	}
	return c;
}

// a launch of fewer members than the persistent grid holds is one wavefront per member.  beside: the small grid (the
// same kernel, fewer wavefronts: every one of them takes more members).  -> the grid of the launch
inline uint32_t launch_compact(const uint8_t *slots, uint64_t stride, const uint32_t *len, const uint64_t *dst_off, uint32_t n,
			       uint8_t *dst, hipStream_t st, bool beside = false)
{
	const uint64_t cus = compact_device_cus();
	uint64_t cap = beside ? cus * COMPACT_BESIDE_WAVES_PER_2CU / 2 : cus * COMPACT_WAVES_PER_CU;
	if (!cap)
		cap = 1;
	const uint32_t grid = n < cap ? n : (uint32_t)cap;
	hipLaunchKernelGGL(k_compact, dim3(grid), dim3(64), 0, st, slots, stride, len, dst_off, n, dst);
	return grid;
}

// RFC 1950 members (HD_FRAME_ZLIB): the Adler-32 of every block's input, written big-endian
// into the last four bytes of its member (lib/zlibutil.c:393-396 computes it on the CPU after
// the codec returns).  Kept out of the encode kernels, which sit at their register budget;
// one extra streaming read of the input, only in this frame.  One wavefront per block.
__global__ __launch_bounds__(64) void k_adler32_patch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
						      uint32_t nblocks, uint8_t *out, uint64_t out_stride,
						      const uint32_t *out_len, const int32_t *status)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= nblocks || (status && status[b]) || out_len[b] < 6)
		return;
	const uint8_t *src = in + in_off[b];
	const uint32_t n = in_len[b];
	const bool aligned = (((uintptr_t)src) & 15) == 0;
	AdlerLanes adl;
	adl.init();
	for (uint32_t piece = 0; piece * HD_PIECE < n; piece++) {
		const uint32_t o = piece * HD_PIECE + lane * 16;
		uint4 v = make_uint4(0, 0, 0, 0);
		if (aligned && o + 16 <= n) {
			v = *(const uint4 *)(src + o);
		} else if (o < n) {
			uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
			for (uint32_t k = 0; k < 16; k++)
				w[k >> 2] |= (o + k < n ? (uint32_t)src[o + k] : 0u) << (8 * (k & 3));
			v = make_uint4(w[0], w[1], w[2], w[3]);
		}
		adl.fold(piece, lane, v);
	}
	const uint32_t a = adl.finish(n);
	if (lane < 4)
		out[(uint64_t)b * out_stride + out_len[b] - 4 + lane] = (uint8_t)(a >> (24 - 8 * lane));
}

} // namespace hd
