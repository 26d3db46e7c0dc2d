// hd_carry.hpp -- a stream cut by SYNC flushes, which keep the 32 KiB window across the cut, decoded in parallel rows.
//
// Role: what zlib's inflate() does with the output of pigz (default mode), of a writer that calls deflate(Z_SYNC_FLUSH), of a
// dictzip-like writer that did not reset the window: one serial decode.  hd_stream.hpp's index finds the flush points of such a
// stream and stops (a row whose matches reach back over its own start does not decode from that start).  Here such a row
// decodes all the same, by the two-pass marker method of pugz / rapidgzip:
//   index   k_carry_piece       hd_inflate_size.hpp's piece decoder without the distance refusal: reach[i] = the furthest a
//                               match of row i goes back over the row's first byte (0: the row stands alone, <= 32768)
//           k_carry_reach_rows  reach[] in row order;  k_carry_cut: the first row with reach[i] > out_off[i] ends the chain
//   decode  k_carry_check_reach the table's reach column is held to reach[i] <= min(32768, out_off[i]) before anything runs
//           k_carry_group       rows whose out_off lies in one multiple of the group size: where they end, their largest reach
//           k_carry_decode      one wavefront per row: the row as SYMBOLS, 16 bits per output byte -- a byte, or
//                               0x8000 | (32768 - backdist) for "the byte backdist in front of this row's start"
//           k_carry_tails       ONE workgroup, rows in order: the last 32 KiB of every row made final against a window in LDS
//           k_carry_resolve     all rows side by side: every other symbol becomes its byte or out[row start - backdist]
//           k_carry_parts / k_carry_crc   the check of the group's bytes in fixed pieces, for hd_stream.hpp's fold
// No kernel waits for another workgroup: what one row needs of another is a kernel boundary, or a barrier in k_carry_tails.
// A group whose largest reach is 0 does not come here at all: it goes through the flush-rule batch inflate into place.
#pragma once
#include "hd_stream.hpp"
#include "hd_deflate_dynamic.hpp"

namespace hd {

constexpr uint32_t CARRY_WINDOW = 32768;                 // DEFLATE's window: the most a distance states
constexpr uint32_t CARRY_MARK = 0x8000u;                 // symbol: bit 15 set = a marker, bits 14..0 = 32768 - backdist
constexpr uint32_t CARRY_CHECK_PIECE = HD_CARRY_CHECK_PIECE;

// ---- the index ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_carry_piece(CarryPieceArgs a) { inflate_size_body<true, CarryPieceArgs, true>(a); }

// the marked candidates' reach in rank order (k_stream_rows writes the other three columns)
__global__ __launch_bounds__(256) void k_carry_reach_rows(const uint32_t *preach, const uint32_t *mark, const uint64_t *rank, uint32_t ncand,
							   uint32_t max_chunks, uint32_t *reach)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i];
	if (r < max_chunks)
		reach[r] = preach[i];
}

// *first (0xffffffff before the launch) = the lowest of the n rows with reach[i] > lim[i], where lim is out_off (the index)
// or min(out_off, 32768) (the decode's check of a caller's table)
__global__ __launch_bounds__(256) void k_carry_check_reach(const uint32_t *reach, const uint64_t *out_off, uint32_t n, uint32_t cap, uint32_t *first)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && (reach[i] > cap || reach[i] > out_off[i]))
		atomicMin(first, i);
}

// the reach rule on k_stream_verdict's sum[]: the first table row that reaches back further than the stream has bytes in
// front of it ends the chain there -- status 1, and the rows in front stay usable
__global__ void k_carry_cut(const uint32_t *first, const uint64_t *in_off, const uint64_t *out_off, uint64_t *sum)
{
	const uint32_t i = *first;
	if (threadIdx.x || i == IDX_NIL)
		return;
	sum[0] = i;
	sum[1] = out_off[i];
	sum[2] = in_off[i];
	sum[3] = 1;
}

// ---- the decode ---------------------------------------------------------------------------------------------------------
// The group that starts at row r0: the rows whose out_off lies in the same multiple of group_bytes as out_off[r0] (a row is
// never split; out_off ascends: k_stream_check_rows).  rec[] = { the row behind the group, the group's largest reach, the
// first output byte of the group, the first behind it }.  One workgroup.
__global__ __launch_bounds__(256) void k_carry_group(const uint64_t *out_off, const uint32_t *out_size, const uint32_t *reach, uint32_t r0,
						      uint32_t n, uint64_t group_bytes, uint64_t *rec)
{
	__shared__ uint32_t s_end, s_max[4];
	const uint32_t t = threadIdx.x;
	if (t == 0) {
		const uint64_t g = out_off[r0] / group_bytes;
		uint32_t lo = r0 + 1, hi = n;                        // the first row behind r0 in another multiple
		while (lo < hi) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (out_off[mid] / group_bytes == g)
				lo = mid + 1;
			else
				hi = mid;
		}
		s_end = lo;
	}
	__syncthreads();
	const uint32_t r1 = s_end;
	uint32_t m = 0;
	for (uint32_t i = r0 + t; i < r1; i += 256)
		m = max(m, reach[i]);
	for (int o = 32; o > 0; o >>= 1)
		m = max(m, (uint32_t)__shfl_down((int)m, o, 64));
	if ((t & 63) == 0)
		s_max[t >> 6] = m;
	__syncthreads();
	if (t == 0) {
		rec[0] = r1;
		rec[1] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
		rec[2] = out_off[r0];
		rec[3] = out_off[r1 - 1] + out_size[r1 - 1];
	}
}

struct CarryDecodeArgs {
	const uint8_t *in;
	const uint64_t *in_off;          // the four tables of the index and its reach column, held to their rules by the caller
	const uint32_t *in_len;
	const uint32_t *out_size;
	const uint64_t *out_off;
	const uint32_t *reach;
	uint32_t r0, nrows;              // the group: rows [r0, r0 + nrows)
	uint64_t base;                   // out_off[r0]: the symbol of output byte q is sym[q - base]
	uint16_t *sym;
	uint32_t *out_len;               // by row: symbols written (0 where the row fails)
	int32_t *status;                 // by row: HD_OK | HD_BAD_DATA | HD_INSUFFICIENT_SPACE
};

// the size pass's tables and stream copy, and the last 32768 symbols of the row: every match source is in LDS
struct CarryLds : InfSizeLds {
	uint16_t ring[CARRY_WINDOW];
};

// One wavefront per row: the size pass's loop (hd_inflate_size.hpp) -- every token through spec_token / window_walk, or
// through the checked scalar path -- with the placement of symbols added.  A symbol goes to the ring and to the scratch; a
// match reads the ring alone, since no distance is longer than the ring, so the wavefront never reads back what it stored.
// The row ends by the flush rule of k_inflate (INF_FLUSHED): behind a final block, or behind a block that uses the last
// input byte.  It may put out at most out_size[row] symbols and reach back at most reach[row] bytes: what the table
// states is checked, not trusted, and a marker is written only for a distance inside that claim.
// The kernel's text is hd_rows_decode.hpp, which makes one kernel per inclusion: this one, and hd_blocks.hpp's for rows that
// start and end on a bit.  Not a template on purpose: with the same text as `template <bool BITS, class Args> __device__
// __forceinline__` body behind two one-line kernels -- the arguments by value or by reference alike -- this kernel compiled to
// 51 VGPRs and 100 SGPRs where the kernel written out has 43 and 99 (gfx950, -O3; the Makefile's resource log shows either),
// and its register line is held to the number.  Measure before turning it back into one.
#define HD_ROWS_DECODE_KERNEL k_carry_decode
#define HD_ROWS_DECODE_ARGS CarryDecodeArgs
#define HD_ROWS_DECODE_BITS false
#include "hd_rows_decode.hpp"

struct CarryRowsArgs {
	const uint16_t *sym;
	uint64_t base;
	const uint64_t *out_off;
	const uint32_t *out_size;
	const uint32_t *out_len;         // k_carry_decode's verdict: a row that failed, or is not out_size long, is left alone
	const int32_t *status;
	uint32_t r0, nrows;
	uint8_t *out;
};

constexpr uint32_t CARRY_TAIL_THREADS = 1024, CARRY_TAIL_PER = CARRY_WINDOW / CARRY_TAIL_THREADS;

// ONE workgroup, the group's rows in order.  ring[q mod 32768] is output byte q for the 32768 bytes in front of the row at
// hand: loaded from `out` at the group's start (the earlier groups are final there), then moved on by every row's TAIL, its
// last min(size, 32768) symbols -- read, resolved against the ring into registers, and only behind a barrier written to the
// ring and to `out`.  A row shorter than the window moves it by its length alone, so a chain of markers runs through any
// number of short rows.  The next row's symbols are requested before this row's are resolved.
__global__ __launch_bounds__(CARRY_TAIL_THREADS) void k_carry_tails(CarryRowsArgs a)
{
	__shared__ uint8_t ring[CARRY_WINDOW];
	const uint32_t t = threadIdx.x;
	for (uint32_t k = t; k < CARRY_WINDOW; k += CARRY_TAIL_THREADS) {
		const uint64_t q = a.base - 1 - k;                   // base - 1 down to base - 32768, where the stream has that many
		if (k < a.base)
			ring[q & (CARRY_WINDOW - 1)] = a.out[q];
	}
	__syncthreads();
	const uint32_t end = a.r0 + a.nrows;
	// the next row at or behind `from` that has a tail: rows of size 0, and rows k_carry_decode refused, have none (uniform)
	auto next_row = [&](uint32_t from) {
		while (from < end && (a.out_size[from] == 0 || a.status[from] != HD_OK || a.out_len[from] != a.out_size[from]))
			from++;
		return from;
	};
	// a row's tail as this thread reads it: symbols j * 1024 + t, two to a register
	auto load_tail = [&](uint32_t row, uint32_t (&x)[CARRY_TAIL_PER / 2]) {
		const uint32_t size = a.out_size[row], tl = size < CARRY_WINDOW ? size : CARRY_WINDOW;
		const uint16_t *s = a.sym + (a.out_off[row] + (size - tl) - a.base);
#pragma unroll
		for (uint32_t j = 0; j < CARRY_TAIL_PER; j += 2) {
			const uint32_t k = j * CARRY_TAIL_THREADS + t;
			x[j / 2] = (k < tl ? (uint32_t)s[k] : 0u) | (k + CARRY_TAIL_THREADS < tl ? (uint32_t)s[k + CARRY_TAIL_THREADS] << 16 : 0u);
		}
	};
	uint32_t cur[CARRY_TAIL_PER / 2] = {}, nxt[CARRY_TAIL_PER / 2] = {};
	uint32_t row = next_row(a.r0);
	if (row < end)
		load_tail(row, cur);
	while (row < end) {
		const uint32_t size = a.out_size[row];
		const uint64_t start = a.out_off[row];
		const uint32_t tl = size < CARRY_WINDOW ? size : CARRY_WINDOW;
		const uint64_t t0 = start + (size - tl);
		// the next row's symbols are on their way while this one is resolved
		const uint32_t follow = next_row(row + 1);
		if (follow < end)
			load_tail(follow, nxt);
		uint32_t v[CARRY_TAIL_PER / 4];                      // the tail's bytes, four to a register
#pragma unroll
		for (uint32_t j = 0; j < CARRY_TAIL_PER; j++) {
			uint32_t x = (cur[j / 2] >> (16 * (j & 1))) & 0xffffu;
			if (x & CARRY_MARK)
				x = ring[(start - (CARRY_WINDOW - (x & (CARRY_MARK - 1)))) & (CARRY_WINDOW - 1)];
			v[j / 4] = (j & 3) ? v[j / 4] | (x << (8 * (j & 3))) : x;
		}
		__syncthreads();
#pragma unroll
		for (uint32_t j = 0; j < CARRY_TAIL_PER; j++) {
			const uint32_t k = j * CARRY_TAIL_THREADS + t;
			if (k < tl) {
				const uint8_t b = (uint8_t)(v[j / 4] >> (8 * (j & 3)));
				ring[(t0 + k) & (CARRY_WINDOW - 1)] = b;
				a.out[t0 + k] = b;
			}
		}
		__syncthreads();
#pragma unroll
		for (uint32_t j = 0; j < CARRY_TAIL_PER / 2; j++)
			cur[j] = nxt[j];
		row = follow;
	}
}

// One workgroup per row, all rows side by side: every symbol in front of the row's tail becomes its byte, or the byte
// backdist in front of the row's start -- which lies in a tail that k_carry_tails made final, in this group or an earlier
// one.  A marker that names a byte in front of the stream cannot come from k_carry_decode; it reads as 0 all the same.
__global__ __launch_bounds__(256) void k_carry_resolve(CarryRowsArgs a)
{
	const uint32_t row = a.r0 + blockIdx.x;
	const uint32_t size = a.out_size[row];
	if (size <= CARRY_WINDOW || a.status[row] != HD_OK || a.out_len[row] != size)
		return;
	const uint64_t start = a.out_off[row];
	const uint16_t *s = a.sym + (start - a.base);
	const uint32_t body = size - CARRY_WINDOW;
	for (uint32_t k = threadIdx.x; k < body; k += 256) {
		uint32_t x = s[k];
		if (x & CARRY_MARK) {
			const uint32_t back = CARRY_WINDOW - (x & (CARRY_MARK - 1));
			x = back <= start ? a.out[start - back] : 0u;
		}
		a.out[start + k] = (uint8_t)x;
	}
}

// the lowest row of [r0, r0 + n) that failed or is not as long as the table states -> *first_bad (atomicMin)
__global__ __launch_bounds__(256) void k_carry_verify(const int32_t *status, const uint32_t *out_len, const uint32_t *out_size, uint32_t r0,
						       uint32_t n, uint32_t *first_bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && (status[r0 + i] != HD_OK || out_len[r0 + i] != out_size[r0 + i]))
		atomicMin(first_bad, r0 + i);
}

// ---- the check of a group's bytes [begin, end), in pieces of CARRY_CHECK_PIECE: a pass of its own behind k_carry_resolve ----
__global__ __launch_bounds__(256) void k_carry_parts(uint64_t begin, uint64_t end, uint32_t np, uint64_t *off, uint32_t *len)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= np)
		return;
	const uint64_t o = begin + (uint64_t)i * CARRY_CHECK_PIECE, left = end - o;
	off[i] = o;
	len[i] = left < CARRY_CHECK_PIECE ? (uint32_t)left : CARRY_CHECK_PIECE;
}

// the CRC-32 of every piece, one wavefront each (k_chunk_adler is the Adler-32's)
__global__ __launch_bounds__(64) void k_carry_crc(const CrcTables *ct, const uint8_t *base, const uint64_t *off, const uint32_t *len, uint32_t np,
						   uint32_t *crc)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= np)
		return;
	const uint32_t c = crc_of_block(ct, base + off[b], len[b], lane);
	if (lane == 0)
		crc[b] = c;
}

} // namespace hd
