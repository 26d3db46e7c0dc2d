// hd_range.hpp -- ranged reads from a container file resident in HBM: decode only the members asked for.
//
// Role: the read a BGZF index exists for -- `bgzip -b OFFSET -s SIZE`, the chunks a .bai / .tbi lookup returns -- on the
// member table of hd_index.hpp.  A batch of queries ([begin, end) in decoded bytes, or in virtual offsets) becomes
//   1. k_range_resolve: one lane per query validates it, finds its decoded span and the first / last member holding a byte
//      of it by binary search, and records the members it covers as +1 / -1 in a difference array;
//   2. k_scan_* over that array, k_range_select: a member is selected where the running count is not zero and it is not
//      empty; two more scans rank the selected members and lay them out back to back in the scratch;
//   3. k_range_tables: row `rank` of the compacted tables batch_inflate_dev and k_members_verify run on;
//   4. k_range_verdict: the first bad row named by the caller's index;
//   5. k_range_gather: a query's members are consecutive in the scratch, so its bytes are ONE run there; the runs are dealt
//      in pieces of HD_RANGE_PIECE bytes over a persistent grid, each piece a compact_wide copy.
// No lane loops over the members or the bytes of a query: a query over the whole file costs what any other does until
// the gather, and there it is spread over the chip.
#pragma once
#include "hd_compact.hpp"
#include "hd_index.hpp"

namespace hd {

constexpr uint32_t RANGE_OK = 0, RANGE_REFUSED = 1, RANGE_TOO_LONG = 2;   // q_status
constexpr uint64_t RANGE_NONE = ~(uint64_t)0;                             // a virtual offset that names no position

// where member m starts in the file: behind its predecessor's trailer (in_len counts the trailer), for every member kind
__device__ __forceinline__ uint64_t range_member_start(const uint64_t *in_off, const uint32_t *in_len, uint32_t m)
{
	return m ? in_off[m - 1] + in_len[m - 1] : 0;
}

// the last m in [0, n) with out_off[m] <= x (out_off[0] == 0).  For x below the total this member is never empty: the
// empty members in front of it share its out_off and come first.
__device__ __forceinline__ uint32_t range_member_of(const uint64_t *out_off, uint32_t n, uint64_t x)
{
	uint32_t lo = 0, hi = n;
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (out_off[mid] <= x)
			lo = mid;
		else
			hi = mid;
	}
	return lo;
}

// U(v): the decoded position a virtual offset names, RANGE_NONE if it names none
__device__ __forceinline__ uint64_t range_voffset(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
						  const uint64_t *out_off, uint32_t n, uint64_t total, uint64_t v)
{
	const uint64_t c = v >> 16;
	const uint32_t u = (uint32_t)v & 0xffffu;
	uint32_t lo = 0, hi = n;                                     // the last m that starts at or before c
	while (hi - lo > 1) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (range_member_start(in_off, in_len, mid) <= c)
			lo = mid;
		else
			hi = mid;
	}
	if (range_member_start(in_off, in_len, lo) == c)
		return u <= out_size[lo] ? out_off[lo] + u : RANGE_NONE;
	if (c == in_off[n - 1] + in_len[n - 1] && u == 0)            // the end of the file
		return total;
	return RANGE_NONE;
}

// one lane per query.  cover[] (nmembers + 1 entries, zero before the launch) receives +1 at the first member of an
// accepted, non-empty query and -1 behind its last (u32 wrap-around: the scan's low 32 bits are the count).
__global__ __launch_bounds__(256) void k_range_resolve(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
							const uint64_t *out_off, uint32_t nmembers, int kind,
							const uint64_t *q_begin, const uint64_t *q_end, uint32_t nqueries,
							uint32_t *q_len, int32_t *q_status, uint32_t *q_pieces, uint32_t *q_first,
							uint64_t *q_from, uint32_t *cover, uint32_t *nrefused)
{
	const uint32_t q = blockIdx.x * 256 + threadIdx.x;
	if (q >= nqueries)
		return;
	const uint64_t total = out_off[nmembers - 1] + out_size[nmembers - 1];
	uint64_t b = q_begin[q], e = q_end[q];
	uint32_t status = RANGE_OK;
	if (kind == HD_RANGE_VOFFSET) {
		b = range_voffset(in_off, in_len, out_size, out_off, nmembers, total, b);
		e = range_voffset(in_off, in_len, out_size, out_off, nmembers, total, e);
		if (b == RANGE_NONE || e == RANGE_NONE || b > e)
			status = RANGE_REFUSED;
	} else {
		if (b > e)
			status = RANGE_REFUSED;
		e = e < total ? e : total;                                   // (begin at or past the total: no bytes, status 0)
	}
	uint64_t len = status == RANGE_OK && b < e ? e - b : 0;
	if (len > 0xffffffffull) {
		status = RANGE_TOO_LONG;
		len = 0;
	}
	uint32_t first = 0;
	if (len) {
		first = range_member_of(out_off, nmembers, b);
		const uint32_t last = range_member_of(out_off, nmembers, e - 1);
		atomicAdd(cover + first, 1u);
		atomicAdd(cover + last + 1, 0xffffffffu);
	}
	if (status != RANGE_OK)
		atomicAdd(nrefused, 1u);
	q_len[q] = (uint32_t)len;
	q_status[q] = (int32_t)status;
	q_pieces[q] = (uint32_t)((len + HD_RANGE_PIECE - 1) / HD_RANGE_PIECE);
	q_first[q] = first;
	q_from[q] = b;
}

// one lane per member: cover_scan[] is the exclusive 64-bit scan of cover[0 .. nmembers], so entry m + 1 holds the sum
// through member m and its low 32 bits are the number of queries that cover m
__global__ __launch_bounds__(256) void k_range_select(const uint64_t *cover_scan, const uint32_t *out_size, uint32_t nmembers,
						       uint32_t *sel, uint32_t *sel_size)
{
	const uint32_t m = blockIdx.x * 256 + threadIdx.x;
	if (m >= nmembers)
		return;
	const uint32_t size = out_size[m];
	const uint32_t s = (uint32_t)cover_scan[m + 1] != 0 && size != 0;
	sel[m] = s;
	sel_size[m] = s ? size : 0;
}

// one lane per member: a selected member's row of the compacted tables, at its rank
__global__ __launch_bounds__(256) void k_range_tables(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
						       const uint32_t *crc_want, const uint32_t *sel, const uint64_t *rank,
						       const uint64_t *scratch_off, uint32_t nmembers, uint64_t *c_in_off,
						       uint32_t *c_in_len, uint64_t *c_out_off, uint32_t *c_out_cap, uint32_t *c_crc_want,
						       uint32_t *c_member)
{
	const uint32_t m = blockIdx.x * 256 + threadIdx.x;
	if (m >= nmembers || !sel[m])
		return;
	const uint64_t r = rank[m];
	c_in_off[r] = in_off[m];
	c_in_len[r] = in_len[m];
	c_out_off[r] = scratch_off[m];
	c_out_cap[r] = out_size[m];
	c_crc_want[r] = crc_want[m];
	c_member[r] = m;
}

// the first bad row of k_members_verify by the caller's index (rows are in member order, so the lowest row is the
// lowest member); nmembers where no row is bad
__global__ void k_range_verdict(const uint32_t *first_bad_row, const uint32_t *c_member, uint32_t nmembers, uint64_t *bad_member)
{
	const uint32_t r = *first_bad_row;
	*bad_member = r == IDX_NIL ? nmembers : c_member[r];
}

// the slice copy.  piece_off[] is the exclusive scan of q_pieces[]; wavefront w takes pieces w, w + grid, ... and finds
// the query of a piece as the last q with piece_off[q] <= piece (a query of no pieces shares its offset with the next
// one and comes first, so it is never found).  Source and destination of a piece may have any alignment: the ragged
// ends are byte stores, so two pieces -- of one query or of two -- never write one another's bytes.
__global__ __launch_bounds__(64) void k_range_gather(const uint8_t *__restrict__ scratch, const uint64_t *__restrict__ scratch_off,
						      const uint64_t *__restrict__ out_off, const uint32_t *__restrict__ q_first,
						      const uint64_t *__restrict__ q_from, const uint32_t *__restrict__ q_len,
						      const uint64_t *__restrict__ dst_off, const uint64_t *__restrict__ piece_off,
						      uint32_t nqueries, uint64_t npieces, uint8_t *__restrict__ dst)
{
	const uint32_t lane = threadIdx.x;
	for (uint64_t p = blockIdx.x; p < npieces; p += gridDim.x) {
		uint32_t lo = 0, hi = nqueries;
		while (hi - lo > 1) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (piece_off[mid] <= p)
				lo = mid;
			else
				hi = mid;
		}
		const uint32_t q = lo, f = q_first[q];
		const uint64_t at = (p - piece_off[q]) * HD_RANGE_PIECE;                 // < q_len[q] < 2^32
		const uint64_t left = q_len[q] - at;
		const uint32_t L = left < HD_RANGE_PIECE ? (uint32_t)left : HD_RANGE_PIECE;
		compact_wide<COMPACT_NT, COMPACT_UNROLL>(scratch + scratch_off[f] + (q_from[q] - out_off[f]) + at, L,
							  dst + dst_off[q] + at, lane);
	}
}

} // namespace hd
