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
__global__ __launch_bounds__(64) void k_carry_decode(CarryDecodeArgs a)
{
	__shared__ CarryLds L;
	const uint32_t lane = threadIdx.x;
	if (blockIdx.x >= a.nrows)
		return;
	const uint32_t row = a.r0 + blockIdx.x;
	const uint32_t n = a.in_len[row];                // < HD_INFLATE_MAX_IN: k_stream_check_rows
	const uint8_t *src = a.in + a.in_off[row];
	const uint32_t cap = a.out_size[row], claim = a.reach[row];
	uint16_t *dst = a.sym + (a.out_off[row] - a.base);

	InfReader R(src, n, lane);
	uint32_t pos = 0;                                // symbols out so far (uniform), <= cap

	// symbols [p, p + length) from `offset` back, the whole wavefront: the source of symbol k is p - offset + (k mod offset),
	// which lies in front of p whatever the overlap; in front of the row's start it is a marker (p - offset + k >= -claim:
	// the caller has checked)
	auto copy = [&](uint32_t p, uint32_t length, uint32_t offset) {
		for (uint32_t k = lane; k < length; k += 64) {
			const int64_t s = (int64_t)p + (k % offset) - offset;
			const uint16_t v = s < 0 ? (uint16_t)(CARRY_MARK | (uint32_t)(CARRY_WINDOW + s)) : L.ring[(uint32_t)s & (CARRY_WINDOW - 1)];
			L.ring[(p + k) & (CARRY_WINDOW - 1)] = v;
			dst[p + k] = v;
		}
	};

	// the literals of a window's lanes in `mask`: lane's byte at its position
	auto put_literals = [&](uint64_t mask, uint32_t p, uint32_t byte) {
		if ((mask >> lane) & 1) {
			L.ring[p & (CARRY_WINDOW - 1)] = (uint16_t)(byte & 0xff);
			dst[p] = (uint16_t)(byte & 0xff);
		}
	};

	// ---- window decode: hd_inflate_size.hpp's, with the tokens' symbols placed.  Returns 0 = one token through the scalar
	// path, 2 = error (st set).
	const uint32_t dw_safe = R.nbytes_al >> 2;
	uint32_t lds_p0 = 0xfffffff0u;
	uint32_t pre_piece = 0, pre_idx = 0xfffffff0u;
	auto run_windows = [&](int32_t &st_out) -> uint32_t {
		uint32_t B = R.bit_pos();
		uint32_t result = 0;
		for (;;) {
			const uint32_t d0 = B >> 5;
			if (!(d0 + 7 <= dw_safe))
				break;
			const uint32_t p0 = d0 >> 6;
			if (p0 != lds_p0) {
				if (p0 == lds_p0 + 1)
					L.comp[lane] = L.comp[64 + lane];
				else
					L.comp[lane] = R.load_piece(p0);
				L.comp[64 + lane] = pre_idx == p0 + 1 ? pre_piece : R.load_piece(p0 + 1);
				pre_piece = R.load_piece(p0 + 2);
				pre_idx = p0 + 2;
				lds_p0 = p0;
			}
			const uint32_t bl0 = (B & 31) + lane;
			const uint32_t *wsp = &L.comp[(d0 & 63) + (bl0 >> 5)];
			const uint32_t ws0 = wsp[0], ws1 = wsp[1], ws2 = wsp[2], ws3 = wsp[3], ws4 = wsp[4];
			const InfSpec s0 = spec_token(L, bl0, ws0, ws1, ws2), s1 = spec_token(L, bl0 + 64, ws2, ws3, ws4);
			uint32_t wb, wm;
			uint64_t real0, real1;
			window_walk(s0.walk, s1.walk, wb, real0, real1, wm);
			if (real0 == 0)
				break;                                     // the token at B is not for a window: scalar path
			const uint32_t scn = wave_incl_scan(sel(real0, s0.outlen, 0u) | (sel(real1, s1.outlen, 0u) << 16));
			const uint32_t tot = readlane(scn, 63);
			const uint32_t total = (tot & 0xffff) + (tot >> 16);
			if (total > cap - pos) {
				st_out = HD_INSUFFICIENT_SPACE;            // more than the table states
				result = 2;
				break;
			}
			const uint32_t opos0 = pos + (scn & 0xffff) - s0.outlen;
			const uint32_t opos1 = pos + (scn >> 16) + (tot & 0xffff) - s1.outlen;
			const uint64_t len0 = real0 & s0.is_len, len1 = real1 & s1.is_len;
			if (pos < CARRY_WINDOW) {
				// further back than the table states for this row: only this early can it be
				const uint64_t far0 = __ballot(opos0 < s0.offset && s0.offset - opos0 > claim);
				const uint64_t far1 = __ballot(opos1 < s1.offset && s1.offset - opos1 > claim);
				if ((far0 & len0) | (far1 & len1)) {
					st_out = HD_BAD_DATA;
					result = 2;
					break;
				}
			}
			// The tokens in stream order: the literals between two matches a lane each, a match by the whole wavefront.  The
			// order is kept strictly -- the ring is exactly as long as the longest distance, so a literal placed ahead of
			// its turn would land on the slot of a byte that a match 32768 - k in front of it still has to read.
			uint64_t lit0 = real0 & s0.is_lit, lit1 = real1 & s1.is_lit;
			for (uint64_t m = len0; m; m &= m - 1) {
				const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1;
				put_literals(lit0 & ((1ull << l) - 1), opos0, s0.length);
				lit0 &= ~((1ull << l) - 1);
				copy(readlane(opos0, l), readlane(s0.length, l), readlane(s0.offset, l));
			}
			put_literals(lit0, opos0, s0.length);
			for (uint64_t m = len1; m; m &= m - 1) {
				const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1;
				put_literals(lit1 & ((1ull << l) - 1), opos1, s1.length);
				lit1 &= ~((1ull << l) - 1);
				copy(readlane(opos1, l), readlane(s1.length, l), readlane(s1.offset, l));
			}
			put_literals(lit1, opos1, s1.length);
			pos += total;
			B += wb;
			if (wm & 64)
				break;                                     // the walk stopped in front of a long codeword or the end of the block
		}
		R.seek_bit(B);
		return result;
	};

	int32_t st = HD_OK;
	bool static_loaded = false;
	for (;;) {
		R.refill();
		lds_p0 = 0xfffffff0u;                     // header parsing reuses the LDS behind L.comp
		const uint32_t bfinal = (uint32_t)R.bb & 1;
		const uint32_t btype = ((uint32_t)R.bb >> 1) & 3;
		R.drop(3);

		if (btype == 0) {
			// ---- stored: the bytes are symbols ------------
			const int64_t cbits = (R.consumed_bits() + 7) & ~(int64_t)7;
			if (cbits > 8 * (int64_t)n) { st = HD_BAD_DATA; break; }
			uint32_t ip = (uint32_t)(cbits >> 3);
			if (n - ip < 4) { st = HD_BAD_DATA; break; }
			R.seek_byte(ip);
			R.refill();
			const uint32_t len = (uint32_t)R.bb & 0xffff, nlen = ((uint32_t)R.bb >> 16) & 0xffff;
			ip += 4;
			if (len != (~nlen & 0xffff)) { st = HD_BAD_DATA; break; }
			if (len > n - ip) { st = HD_BAD_DATA; break; }
			if (len > cap - pos) { st = HD_INSUFFICIENT_SPACE; break; }
			for (uint32_t k = lane; k < len; k += 64) {
				const uint16_t v = src[ip + k];
				L.ring[(pos + k) & (CARRY_WINDOW - 1)] = v;
				dst[pos + k] = v;
			}
			pos += len;
			R.seek_byte(ip + len);
		} else if (btype == 3) {
			st = HD_BAD_DATA;
			break;
		} else {
			if (btype == 2) {
				if (!inflate_dynamic_header(R, L, n, lane)) { st = HD_BAD_DATA; break; }
				static_loaded = false;
			} else if (!static_loaded) {
				inflate_static_tables(L, lane);
				static_loaded = true;
			}

			// ---- symbol loop ----------------------------------------------
			for (;;) {
				if (uniform(run_windows(st)))
					break;
				// one token through the fully checked scalar path (stream edges, long codes, end of block): the size pass's copy
				R.refill();
				if (R.overrun()) { st = HD_BAD_DATA; break; }
				uint32_t e = uniform(L.lit[(uint32_t)R.bb & ((1u << INF_LT_BITS) - 1)]);
				if (((e >> 8) & 3) == K_SLOW) {
					const uint32_t sl = uniform(slow_decode(R.bb, L.lit_count, L.lit_sorted, lane));
					e = litlen_entry(sl & 0xffff, sl >> 16);
				}
				R.drop(e & 15);
				const uint32_t kind = (e >> 8) & 3;
				if (kind == K_LIT) {
					if (pos == cap) { st = HD_INSUFFICIENT_SPACE; break; }
					if (lane == 0) {
						L.ring[pos & (CARRY_WINDOW - 1)] = (uint16_t)(e >> 16);
						dst[pos] = (uint16_t)(e >> 16);
					}
					pos++;
					continue;
				}
				if (kind == K_EOB)
					break;
				const uint32_t eb = (e >> 4) & 15;
				const uint32_t length = (e >> 16) + ((uint32_t)R.bb & ((1u << eb) - 1));
				R.drop(eb);
				if (length > cap - pos) { st = HD_INSUFFICIENT_SPACE; break; }
				R.refill();
				uint32_t d = uniform(L.off[(uint32_t)R.bb & ((1u << INF_DT_BITS) - 1)]);
				if (((d >> 8) & 3) == K_SLOW) {
					const uint32_t sl = uniform(slow_decode(R.bb, L.off_count, L.off_sorted, lane));
					d = offset_entry(sl & 0xffff, sl >> 16);
				}
				const uint32_t deb = (d >> 4) & 15;
				R.drop(d & 15);
				const uint32_t offset = (d >> 16) + ((uint32_t)R.bb & ((1u << deb) - 1));
				R.drop(deb);
				if (offset > pos && offset - pos > claim) { st = HD_BAD_DATA; break; }       // further back than the table states
				copy(pos, length, offset);
				pos += length;
			}
			if (st != HD_OK)
				break;
		}
		if (bfinal)
			break;
		if (R.consumed_bits() <= 8 * (int64_t)n && R.consumed_bits() + 7 >= 8 * (int64_t)n)
			break;                                    // the flush rule: every input byte is used
		if (R.consumed_bits() > 8 * (int64_t)n + 64) { st = HD_BAD_DATA; break; }
	}
	if (st == HD_OK && R.consumed_bits() > 8 * (int64_t)n)
		st = HD_BAD_DATA;
	if (lane == 0) {
		a.out_len[row] = st == HD_OK ? pos : 0u;
		a.status[row] = st;
	}
}

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
