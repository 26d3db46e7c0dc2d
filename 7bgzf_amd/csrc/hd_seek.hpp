// hd_seek.hpp -- a seek index for one stream: the window in front of every row, kept once, and ranged reads on it.
//
// Role: what zran, gztool and rapidgzip call an index with windows, on the row tables of hd_carry.hpp (byte rows) and
// hd_blocks.hpp (bit rows).  A row of either table names bytes in front of itself only within reach[i], and k_carry_decode /
// k_blocks_decode turn every such reference into a marker that points straight into those reach[i] bytes -- a match whose
// source is a marker copies the marker -- so every symbol of a row is a byte or a direct index into the window in front of
// the row.  With the reach[i] bytes in front of every row kept, behind one full decode, every row stands alone:
//   windows  k_seek_check_out   the output-side columns held to their rules (with k_carry_check_reach)
//            k_seek_windows     one wavefront per row: out[out_off - reach, out_off) -> win[win_off, win_off + reach), a compact_wide copy
//            and k_scan_* for win_off, k_carry_crc for the CRC-32 of every row's bytes
//   read     k_seek_check_win   win_off held to the reach column and to win_bytes (the other columns: the decode calls' checks)
//            k_range_resolve .. k_range_select   the queries, as the member call resolves them (hd_range.hpp)
//            k_seek_tables      row `rank` of the compacted tables, a selected row's seven columns
//            k_carry_decode / k_blocks_decode    the selected rows as symbols, group by group, as the kernels stand
//            k_seek_resolve     all rows of the group side by side, no order between them: a symbol becomes its byte or
//                               win[win_off + reach - backdist], eight symbols to a 16-byte load and eight bytes to a store
//            k_carry_verify, k_carry_crc + k_seek_check_crc, k_range_verdict, k_range_gather
// No kernel waits for another workgroup, and none walks the rows in order: there is no tails pass.
#pragma once
#include "hd_range.hpp"
#include "hd_blocks.hpp"

namespace hd {

// ---- the windows --------------------------------------------------------------------------------------------------------
// one lane per row: out_off is the exclusive prefix sum of out_size from 0 and ends at out_bytes.  *bad (0xffffffff before
// the launch) takes the lowest row at fault.  (The reach column: k_carry_check_reach.)
__global__ __launch_bounds__(256) void k_seek_check_out(const uint32_t *out_size, const uint64_t *out_off, uint32_t n, uint64_t out_bytes,
							 uint32_t *bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t q = out_off[i], next = i + 1 < n ? out_off[i + 1] : out_bytes;
	if ((i == 0 && q != 0) || next < q || next - q != out_size[i])
		atomicMin(bad, i);
}

// one wavefront per row, a persistent grid: the reach[i] bytes in front of row i, to win + win_off[i].  The caller has held
// reach[i] <= min(32768, out_off[i]) and win_off to the prefix sum of reach, whose total fits the room.
__global__ __launch_bounds__(64) void k_seek_windows(const uint8_t *__restrict__ out, const uint64_t *__restrict__ out_off,
						      const uint32_t *__restrict__ reach, const uint64_t *__restrict__ win_off, uint32_t n,
						      uint8_t *__restrict__ win)
{
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
		const uint32_t r = reach[i];
		if (r)
			compact_wide<COMPACT_NT, COMPACT_UNROLL>(out + (out_off[i] - r), r, win + win_off[i], lane);
	}
}

// ---- the ranged read ----------------------------------------------------------------------------------------------------
// one lane per row: win_off[0] == 0, row i's window is reach[i] long and ends at or in front of win_bytes.  *bad takes the
// lowest row at fault (a table whose windows are right but longer than win_bytes together: the first row whose window
// ends behind win_bytes).
__global__ __launch_bounds__(256) void k_seek_check_win(const uint64_t *win_off, const uint32_t *reach, uint32_t n, uint64_t win_bytes,
							 uint32_t *bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t w = win_off[i], next = win_off[i + 1];
	if ((i == 0 && w != 0) || next < w || next - w != reach[i] || next > win_bytes)
		atomicMin(bad, i);
}

// the compacted tables of a read: c.x[rank] = x[row] for every selected row
struct SeekColumns {
	uint64_t *in_off, *out_off, *win_off;
	uint32_t *in_len, *out_size, *reach, *row_check, *row;
};

// one lane per row: a selected row's columns at its rank.  out_off becomes the row's place in the byte scratch, the prefix
// sum of the selected sizes (row_check: NULL where the caller keeps none).
__global__ __launch_bounds__(256) void k_seek_tables(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
						      const uint32_t *reach, const uint64_t *win_off, const uint32_t *row_check,
						      const uint32_t *sel, const uint64_t *rank, const uint64_t *scratch_off, uint32_t n, SeekColumns c)
{
	const uint32_t m = blockIdx.x * 256 + threadIdx.x;
	if (m >= n || !sel[m])
		return;
	const uint64_t r = rank[m];
	c.in_off[r] = in_off[m];
	c.in_len[r] = in_len[m];
	c.out_size[r] = out_size[m];
	c.out_off[r] = scratch_off[m];
	c.reach[r] = reach[m];
	c.win_off[r] = win_off[m];
	c.row_check[r] = row_check ? row_check[m] : 0u;
	c.row[r] = m;
}

constexpr uint32_t SEEK_PIECE = 4096;            // bytes of the byte scratch a wavefront of k_seek_resolve takes: eight trips of 64 lanes x 8

struct SeekResolveArgs {
	const uint16_t *sym;             // the group's symbols: the symbol of scratch byte q is sym[q - base]
	uint64_t base, end;              // the group's bytes in the scratch: [base, end)
	const uint64_t *out_off;         // the compacted tables; the group is rows [r0, r0 + nrows), none of them empty
	const uint32_t *out_size;
	const uint32_t *reach;
	const uint64_t *win_off;
	uint32_t r0, nrows;
	const uint8_t *win;
	uint8_t *out;                    // the byte scratch, 16-byte aligned
};

// the last r in [lo, hi] with out_off[r] <= x (out_off[lo] <= x)
__device__ __forceinline__ uint32_t seek_row_of(const uint64_t *out_off, uint32_t lo, uint32_t hi, uint64_t x)
{
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo + 1) >> 1);
		if (out_off[mid] <= x)
			lo = mid;
		else
			hi = mid - 1;
	}
	return lo;
}

// One wavefront per SEEK_PIECE bytes of the byte scratch, counted from a multiple of SEEK_PIECE: a lane takes the eight
// bytes at a multiple of 8, their symbols by one 16-byte load (of whatever alignment the group's base gives it), the bytes
// by one 8-byte store.  Where the eight hold a marker, lie in more than one row, or straddle an end of the group, the lane
// goes symbol by symbol: a marker of row r is win[win_off[r] + reach[r] - backdist], and one that names a byte further back
// than reach[r] -- k_carry_decode writes none; a row it refused may hold what an earlier call left -- reads as 0 and touches
// no memory.  The piece's first and last row by binary search (uniform); a lane searches between the two only where they differ.
__global__ __launch_bounds__(64) void k_seek_resolve(SeekResolveArgs a)
{
	const uint32_t lane = threadIdx.x;
	const uint64_t p0 = ((a.base / SEEK_PIECE) + blockIdx.x) * SEEK_PIECE;
	const uint64_t lo_q = p0 > a.base ? p0 : a.base, hi_q = p0 + SEEK_PIECE < a.end ? p0 + SEEK_PIECE : a.end;
	if (lo_q >= hi_q)
		return;
	const uint32_t last = a.r0 + a.nrows - 1;
	const uint32_t row_lo = seek_row_of(a.out_off, a.r0, last, lo_q), row_hi = seek_row_of(a.out_off, row_lo, last, hi_q - 1);
	for (uint32_t trip = 0; trip < SEEK_PIECE / 512; trip++) {
		const uint64_t q = p0 + 512 * trip + 8 * lane;
		const uint64_t from = q > lo_q ? q : lo_q, to = q + 8 < hi_q ? q + 8 : hi_q;
		if (from >= to)
			continue;
		uint32_t w[4] = { 0, 0, 0, 0 };
		const bool whole = from == q && to == q + 8;
		if (whole) {
			const compact_u32x4 v = *(const compact_u32x4_any *)(a.sym + (q - a.base));
			w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
		} else {
#pragma unroll
			for (uint32_t k = 0; k < 8; k++)
				if (q + k >= from && q + k < to)
					w[k >> 1] |= (uint32_t)a.sym[q + k - a.base] << (16 * (k & 1));
		}
		uint32_t r = row_lo == row_hi ? row_lo : seek_row_of(a.out_off, row_lo, row_hi, from);
		uint64_t row_end = a.out_off[r] + a.out_size[r];
		if (whole && q + 8 <= row_end && !((w[0] | w[1] | w[2] | w[3]) & 0x80008000u)) {
			uint2 b;
			b.x = __builtin_amdgcn_perm(w[1], w[0], 0x06040200u);
			b.y = __builtin_amdgcn_perm(w[3], w[2], 0x06040200u);
			*(uint2 *)(a.out + q) = b;
			continue;
		}
#pragma unroll
		for (uint32_t k = 0; k < 8; k++) {
			const uint64_t at = q + k;
			if (at < from || at >= to)
				continue;
			while (at >= row_end && r < last) {              // (rows are not empty: at most a row a byte)
				r++;
				row_end = a.out_off[r] + a.out_size[r];
			}
			uint32_t x = (w[k >> 1] >> (16 * (k & 1))) & 0xffffu;
			if (x & CARRY_MARK) {
				const uint32_t back = CARRY_WINDOW - (x & (CARRY_MARK - 1)), have = a.reach[r];
				x = back <= have ? a.win[a.win_off[r] + (have - back)] : 0u;
			}
			a.out[at] = (uint8_t)x;
		}
	}
}

// one lane per selected row: the CRC-32 of its bytes against the one the caller keeps -> the lowest rank that differs
__global__ __launch_bounds__(256) void k_seek_check_crc(const uint32_t *crc, const uint32_t *want, uint32_t n, uint32_t *first_bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && crc[i] != want[i])
		atomicMin(first_bad, i);
}

} // namespace hd
