// hd_index.hpp -- member table of a device-resident stream of gzip members.
//
// Role: the serial header walk in front of every decode -- _read_gz_header per member (applet/7bgzf.c:81-131) inside
// the read loop of applet/7bgzf.c:306-328; member_len() of hd_bgzf_host.c and bgzf_scan() of the Python view are its
// host forms -- for a file that lives in HBM.  The walk is a chain (a member's length says where the next one starts),
// so the device form is speculative:
//   1. k_index_flag / k_index_write: one streaming read of the blob finds every position that CAN start a member
//      (1f 8b 08, FLG with FEXTRA and no reserved bit) and compacts them into a sorted list;
//   2. k_index_links: one lane per candidate applies the member_len() rules and resolves "p + total" to a candidate;
//   3. k_index_jump: pointer doubling marks the candidates reachable from the one at offset 0 -- the true chain;
//   4. k_members_tables: the marked candidates, ranked by a prefix count, become the four tables of batch_inflate_dev;
//   5. k_index_verdict names where the walk stopped and why.
// k_members_verify is the trailer check behind the inflate (applet/7bgzf.c:340-352 on the host).
// The second half of the file is the same walk for members that state no length (hipdeflate_index_members_any_dev): the
// matcher without the FEXTRA requirement, and a links pass that sizes such a member by decoding it (k_inflate_member).
// Every read of the blob is bounded by nbytes, whatever the blob says.
#pragma once
#include "hd_compact.hpp"
#include "hd_frame.hpp"
#include "hd_inflate_size.hpp"

namespace hd {

constexpr uint32_t IDX_WORD = 1024;                  // blob bytes per bitmap word: one wavefront load of 64 x 16 bytes
constexpr uint32_t IDX_TILE_WORDS = 256;             // bitmap words per workgroup: the write pass gives each thread one
constexpr uint32_t IDX_TILE = IDX_WORD * IDX_TILE_WORDS;
constexpr uint32_t IDX_NIL = 0xffffffffu;            // no successor: the link ends at nbytes, or it is bad
constexpr uint32_t MEMBER_OK = 0, MEMBER_BAD = 1, MEMBER_CUT = 2;     // (= hipdeflate_member_summary.status 0 / 1 / 2)

// the 16 bytes at o and the 4 behind them (a magic may straddle the granule); bytes at and behind nbytes read as 0,
// which never completes a magic (FLG must have bit 2 set)
__device__ __forceinline__ void index_load20(const uint8_t *blob, uint64_t nbytes, uint64_t o, uint32_t (&d)[5])
{
	if (o + 20 <= nbytes) {
		const uint4 v = *(const uint4 *)(blob + o);
		d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
		d[4] = *(const uint32_t *)(blob + o + 16);
	} else {
		d[0] = d[1] = d[2] = d[3] = d[4] = 0;
#pragma unroll
		for (uint32_t k = 0; k < 20; k++)
			d[k >> 2] |= (o + k < nbytes ? (uint32_t)blob[o + k] : 0u) << (8 * (k & 3));
	}
}

// bit k: the four bytes at o + k, as a little-endian word w, have (w & MASK) == WANT
template <uint32_t MASK, uint32_t WANT> __device__ __forceinline__ uint32_t index_match16_of(const uint32_t (&d)[5])
{
	uint32_t m = 0;
#pragma unroll
	for (uint32_t k = 0; k < 16; k++) {
		const uint32_t w = (k & 3) ? __builtin_amdgcn_alignbyte(d[(k >> 2) + 1], d[k >> 2], k & 3) : d[k >> 2];
		m |= (uint32_t)((w & MASK) == WANT) << k;
	}
	return m;
}

// bit k: the four bytes at o + k are 1f 8b 08 FLG with FLG & 0xe4 == 0x04
__device__ __forceinline__ uint32_t index_match16(const uint32_t (&d)[5]) { return index_match16_of<0xe4ffffffu, 0x04088b1fu>(d); }

// The matcher of the two passes is a parameter: m(d, o) = the bits k of the granule at o whose position o + k matches, and
// a match at position q makes the candidate q + M::SHIFT.  MatchMember is the member index's: a candidate is where the
// gzip magic starts.  (hd_stream.hpp has the other one.)
struct MatchMember {
	static constexpr uint32_t SHIFT = 0;
	__device__ __forceinline__ uint32_t operator()(const uint32_t (&d)[5], uint64_t) const { return index_match16(d); }
};

// pass 1: per 1 KiB word a ballot of the 16-byte granules that hold a candidate, per tile the candidate count
template <class M>
__device__ __forceinline__ void index_flag_body(const uint8_t *blob, uint64_t nbytes, uint64_t *bitmap, uint32_t *tile_cnt, const M &match)
{
	__shared__ uint32_t wcnt[4];
	const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
	const uint64_t word0 = (uint64_t)blockIdx.x * IDX_TILE_WORDS + w * (IDX_TILE_WORDS / 4);
	uint32_t cnt = 0;
#pragma unroll 4
	for (uint32_t it = 0; it < IDX_TILE_WORDS / 4; it++) {
		const uint64_t base = (word0 + it) * IDX_WORD;
		if (base >= nbytes)
			break;
		uint32_t d[5];
		index_load20(blob, nbytes, base + lane * 16, d);
		const uint32_t m = match(d, base + lane * 16);
		cnt += __popc(m);
		const uint64_t any = __ballot(m != 0);
		if (lane == 0)
			bitmap[word0 + it] = any;
	}
	for (int o = 32; o > 0; o >>= 1)
		cnt += (uint32_t)__shfl_down((int)cnt, o, 64);
	if (lane == 0)
		wcnt[w] = cnt;
	__syncthreads();
	if (t == 0)
		tile_cnt[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// pass 2: thread t of tile b owns bitmap word b * 256 + t; it re-reads the flagged granules only, and the candidates
// of the tile go to pos[tile_off[b]...] in ascending order
template <class M>
__device__ __forceinline__ void index_write_body(const uint8_t *blob, uint64_t nbytes, const uint64_t *bitmap, uint64_t nwords,
						 const uint64_t *tile_off, uint64_t *pos, const M &match)
{
	__shared__ uint32_t wtot[4];
	const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
	const uint64_t wi = (uint64_t)blockIdx.x * IDX_TILE_WORDS + t;
	const uint64_t bits = wi < nwords ? bitmap[wi] : 0;
	uint32_t c = 0;
	for (uint64_t b = bits; b; b &= b - 1) {
		const uint64_t o = wi * IDX_WORD + (uint32_t)__ffsll((long long)b) * 16 - 16;
		uint32_t d[5];
		index_load20(blob, nbytes, o, d);
		c += __popc(match(d, o));
	}
	const uint32_t incl = wave_incl_scan(c);
	if (lane == 63)
		wtot[w] = incl;
	__syncthreads();
	uint64_t at = tile_off[blockIdx.x] + (incl - c);
	for (uint32_t k = 0; k < w; k++)
		at += wtot[k];
	for (uint64_t b = bits; b; b &= b - 1) {
		const uint64_t o = wi * IDX_WORD + (uint32_t)__ffsll((long long)b) * 16 - 16;
		uint32_t d[5];
		index_load20(blob, nbytes, o, d);
		for (uint32_t m = match(d, o); m; m &= m - 1)
			pos[at++] = o + (uint32_t)__ffs((int)m) - 1 + M::SHIFT;
	}
}

__global__ __launch_bounds__(256) void k_index_flag(const uint8_t *blob, uint64_t nbytes, uint64_t *bitmap, uint32_t *tile_cnt)
{
	index_flag_body(blob, nbytes, bitmap, tile_cnt, MatchMember{});
}

__global__ __launch_bounds__(256) void k_index_write(const uint8_t *blob, uint64_t nbytes, const uint64_t *bitmap,
						      uint64_t nwords, const uint64_t *tile_off, uint64_t *pos)
{
	index_write_body(blob, nbytes, bitmap, nwords, tile_off, pos, MatchMember{});
}

struct Member {
	uint32_t cls, hdr, total;            // MEMBER_OK: header bytes and whole member, p + total <= nbytes
};

__device__ __forceinline__ uint32_t index_rd16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t index_rd32(const uint8_t *p) { return index_rd16(p) | index_rd16(p + 2) << 16; }

// member_len() of hd_bgzf_host.c at position p < nbytes, with its refusals told apart: MEMBER_BAD where the bytes that
// are there rule a member out, MEMBER_CUT where they run out first (the header, a name without its NUL, the member).
// The FNAME / FCOMMENT scan is the one loop here the blob sizes.  With CLASSIFY (k_index_verdict, one lane) the checks
// come in member_len()'s order, so an unknown extra field behind an endless name is CUT.  Without it (k_index_links,
// every candidate) only BAD-or-CUT against OK matters, and an extra field of no known kind is refused before the name
// is scanned.  A candidate that does scan has XLEN < 256, i.e. a zero byte at p + 11, and starts at most 32 bytes in,
// so each of its two scans ends at or before the zero of the next scanning candidate 21 or more bytes ahead; only the
// few candidates within 21 bytes of one another share a stretch, and only the last few can run to nbytes.  All name
// scans together read O(nbytes), however many decoys the blob holds; one lane still reads one long name byte by byte.
template <bool CLASSIFY>
__device__ inline Member member_parse(const uint8_t *blob, uint64_t p, uint64_t nbytes)
{
	const uint64_t avail = nbytes - p;
	const uint8_t *b = blob + p;
	Member r = { MEMBER_BAD, 0, 0 };
	if ((avail > 0 && b[0] != 0x1f) || (avail > 1 && b[1] != 0x8b) || (avail > 2 && b[2] != 8) ||
	    (avail > 3 && ((b[3] & 0xe0) || !(b[3] & 4))))
		return r;
	r.cls = MEMBER_CUT;
	if (avail < 12)
		return r;
	const uint32_t flg = b[3], xlen = index_rd16(b + 10);
	if (avail < 12 + (uint64_t)xlen)
		return r;
	const uint8_t *x = b + 12;
	const uint32_t tag = xlen >= 4 ? index_rd32(x) : 0;
	uint64_t t = 0;
	bool mz = false, known = true;
	if (xlen == 6 && tag == 0x00024342u)                         // BC 02 00
		t = (uint64_t)index_rd16(x + 4) + 1;
	else if (xlen == 8 && tag == 0x00045a4du)                    // MZ 04 00: + header + trailer, below
		t = index_rd32(x + 4), mz = true;
	else if (xlen == 20 && tag == 0x00104749u)                   // IG 10 00
		t = (uint64_t)index_rd32(x + 4) | (uint64_t)index_rd32(x + 8) << 32;
	else if (xlen == 8 && tag == 0x00044749u)                    // IG 04 00
		t = index_rd32(x + 4);
	else if (xlen == 4 && (tag >> 24) == 0x7d)                   // mgzip
		t = tag & 0xffffffu;
	else
		known = false;
	if (!CLASSIFY && !known) {
		r.cls = MEMBER_BAD;
		return r;
	}
	uint64_t n = 12 + xlen;
	for (uint32_t bit = 0x08; bit <= 0x10; bit <<= 1) {          // FNAME, FCOMMENT
		if (!(flg & bit))
			continue;
		for (;;) {
			if (n >= avail)
				return r;
			if (!b[n++])
				break;
		}
	}
	if (flg & 0x02)                                              // FHCRC
		n += 2;
	if (n > avail)
		return r;
	if (mz)
		t += n + 8;
	if (!known || t < n + 8 || t > 0xfffffff0u) {
		r.cls = MEMBER_BAD;
		return r;
	}
	if (t > avail)
		return r;
	r.cls = MEMBER_OK;
	r.hdr = (uint32_t)n;
	r.total = (uint32_t)t;
	return r;
}

// one lane per candidate: its member (total 0 = none) and the candidate its end points at.  Links go strictly forward.
__global__ __launch_bounds__(256) void k_index_links(const uint8_t *blob, uint64_t nbytes, const uint64_t *pos, uint32_t ncand,
						      uint32_t *succ, uint32_t *hdr, uint32_t *total, uint32_t *mark)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	const uint64_t p = pos[i];
	const Member m = member_parse<false>(blob, p, nbytes);
	uint32_t s = IDX_NIL;
	if (m.cls == MEMBER_OK) {
		const uint64_t next = p + m.total;
		uint32_t lo = i + 1, hi = ncand;
		while (lo < hi) {
			const uint32_t mid = lo + ((hi - lo) >> 1);
			if (pos[mid] < next)
				lo = mid + 1;
			else
				hi = mid;
		}
		if (lo < ncand && pos[lo] == next)
			s = lo;
	}
	succ[i] = s;
	hdr[i] = m.hdr;
	total[i] = m.total;
	mark[i] = i == 0 && p == 0 && m.total;               // the head of the true chain
}

// one round of pointer doubling.  in[] holds every candidate's 2^k-th successor and the marked set holds the members
// at distance < 2^k from the head: a marked candidate marks its 2^k-th successor (a member: candidates without one are
// never marked and end the chain), so the set grows to distance < 2^(k+1); out[] = the 2^(k+1)-th successors.  A mark
// set in this round and already seen by another lane only marks a member further down the same chain.
__global__ __launch_bounds__(256) void k_index_jump(const uint32_t *in, uint32_t *out, const uint32_t *total, uint32_t *mark,
						     uint32_t ncand)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	const uint32_t s = in[i];
	uint32_t s2 = IDX_NIL;
	if (s != IDX_NIL) {
		if (mark[i] && total[s])
			mark[s] = 1;
		s2 = in[s];
	}
	out[i] = s2;
}

// the marked candidates in rank order (rank = exclusive prefix count of the marks) -> the tables; the last one says
// where the walk stopped
__global__ __launch_bounds__(256) void k_members_tables(const uint8_t *blob, const uint64_t *pos, const uint32_t *hdr,
							 const uint32_t *total, const uint32_t *mark, const uint64_t *rank,
							 uint32_t ncand, uint64_t nrows, uint32_t max_members, uint64_t *in_off,
							 uint32_t *in_len, uint32_t *out_size, uint32_t *crc_want, uint64_t *end_offset)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i], p = pos[i];
	const uint32_t h = hdr[i], t = total[i];
	if (r < max_members) {
		in_off[r] = p + h;
		in_len[r] = t - h;
		crc_want[r] = index_rd32(blob + p + t - 8);
		out_size[r] = index_rd32(blob + p + t - 4);
	}
	if (r + 1 == nrows)
		*end_offset = p + t;
}

// sum[] = { nmembers, out_bytes, end_offset, status }
__global__ void k_index_verdict(const uint8_t *blob, uint64_t nbytes, uint64_t nrows, uint32_t max_members, uint64_t *sum)
{
	const uint64_t end = sum[2];
	uint64_t status = 0;
	if (end < nbytes)
		status = member_parse<true>(blob, end, nbytes).cls == MEMBER_CUT ? MEMBER_CUT : MEMBER_BAD;
	if (nrows > max_members)
		status = 3;
	sum[0] = nrows;
	sum[3] = status;
}

// first member whose inflate result disagrees with its trailer: one atomic per workgroup
__global__ __launch_bounds__(256) void k_members_verify(const int32_t *status, const uint32_t *out_len, const uint32_t *crc,
							 const uint32_t *out_size, const uint32_t *crc_want, uint32_t n,
							 uint32_t *first_bad)
{
	__shared__ uint32_t wmin[4];
	const uint32_t t = threadIdx.x, i = blockIdx.x * 256 + t;
	uint32_t v = IDX_NIL;
	if (i < n && (status[i] != 0 || out_len[i] != out_size[i] || crc[i] != crc_want[i]))
		v = i;
	for (int o = 32; o > 0; o >>= 1)
		v = min(v, (uint32_t)__shfl_down((int)v, o, 64));
	if ((t & 63) == 0)
		wmin[t >> 6] = v;
	__syncthreads();
	if (t == 0) {
		v = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
		if (v != IDX_NIL)
			atomicMin(first_bad, v);
	}
}

/* ---- members that state no length (hipdeflate_index_members_any_dev) ----
   The walk above over blob[lo, n): a candidate is any 1f 8b 08 FLG without a reserved bit, all four bytes in front of n.
   A member whose extra field is one of the five known kinds is member_parse's, to the bit (rule A); every other one is
   sized by decoding it without output inside its window of max_in bytes (rule B: k_member_open, k_inflate_member).  The
   links pass is therefore two steps with the sizing of the compacted rule-B subset between them:
     k_any_classify -> scan, k_any_compact -> k_member_open, k_inflate_member -> k_any_links -> k_index_jump ... as above. */

constexpr uint32_t MEMBER_LONG = 4;                  // (= hipdeflate_member_any_summary.status 4)

// positions o + k >= lo (lo < 16: the call starts the pass on the granule that holds it) whose four bytes end at or before n
// -- index_load20's zeros behind n would complete a magic with FLG 0
struct MatchAny {
	uint64_t lo, n;
	static constexpr uint32_t SHIFT = 0;
	__device__ __forceinline__ uint32_t operator()(const uint32_t (&d)[5], uint64_t o) const
	{
		uint32_t m = index_match16_of<0xe0ffffffu, 0x00088b1fu>(d);
		if (o < lo)
			m &= 0xffffu << (uint32_t)(lo - o);
		if (o + 20 > n)
			m &= o + 4 > n ? 0u : (1u << (uint32_t)(n - o - 3)) - 1;
		return m;
	}
};

__global__ __launch_bounds__(256) void k_any_flag(const uint8_t *blob, uint64_t nbytes, uint64_t lo, uint64_t *bitmap, uint32_t *tile_cnt)
{
	index_flag_body(blob, nbytes, bitmap, tile_cnt, MatchAny{ lo, nbytes });
}

__global__ __launch_bounds__(256) void k_any_write(const uint8_t *blob, uint64_t nbytes, uint64_t lo, const uint64_t *bitmap,
						    uint64_t nwords, const uint64_t *tile_off, uint64_t *pos)
{
	index_write_body(blob, nbytes, bitmap, nwords, tile_off, pos, MatchAny{ lo, nbytes });
}

// rule A applies: FEXTRA, and XLEN and the tag are those of one of the five kinds, by member_parse's tests
__device__ __forceinline__ bool member_states_length(const uint8_t *blob, uint64_t p, uint64_t nbytes)
{
	const uint64_t avail = nbytes - p;
	const uint8_t *b = blob + p;
	if (!(b[3] & 4) || avail < 12)
		return false;
	const uint32_t xlen = index_rd16(b + 10);
	if ((xlen != 4 && xlen != 6 && xlen != 8 && xlen != 20) || avail < 12 + (uint64_t)xlen)
		return false;
	const uint32_t tag = index_rd32(b + 12);
	return (xlen == 6 && tag == 0x00024342u) || (xlen == 8 && (tag == 0x00045a4du || tag == 0x00044749u)) ||
	       (xlen == 20 && tag == 0x00104749u) || (xlen == 4 && (tag >> 24) == 0x7d);
}

// step 1, one lane per candidate: rule A decides at once (cls, hdr, total); rule B marks the candidate to be sized
__global__ __launch_bounds__(256) void k_any_classify(const uint8_t *blob, uint64_t nbytes, const uint64_t *pos, uint32_t ncand,
						       uint32_t *cls, uint32_t *hdr, uint32_t *total, uint32_t *osize, uint32_t *tosize)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	const uint64_t p = pos[i];
	const bool a = member_states_length(blob, p, nbytes);
	Member m = { MEMBER_BAD, 0, 0 };
	if (a)
		m = member_parse<true>(blob, p, nbytes);
	cls[i] = m.cls;
	hdr[i] = m.hdr;
	total[i] = m.total;
	osize[i] = 0;
	tosize[i] = !a;
}

// the rule-B subset, ascending: sub[rank[i]] = i
__global__ __launch_bounds__(256) void k_any_compact(const uint32_t *tosize, const uint64_t *rank, uint32_t ncand, uint32_t *sub)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < ncand && tosize[i])
		sub[rank[i]] = i;
}

// One wavefront per candidate to size: its header by k_frame_open's gzip rules, read in stream order inside the window
// [p, p + min(nbytes - p, max_in)).  status HD_OK: hdr[] bytes of header, and at least one byte of the window behind them;
// PIECE_CUT: a header byte, or the stream's first, lies at or behind the window's end.  Nothing in a header is BAD: the
// matcher saw the magic and FLG.  The names are scanned by all 64 lanes.
__global__ __launch_bounds__(64) void k_member_open(const uint8_t *blob, uint64_t nbytes, const uint64_t *pos, const uint32_t *sub,
						     uint32_t nsub, uint32_t max_in, uint32_t *hdr, int32_t *status)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= nsub)
		return;
	const uint32_t row = sub[b];
	const uint64_t p = pos[row], left = nbytes - p;
	const uint32_t n = left < max_in ? (uint32_t)left : max_in;
	const uint8_t *src = blob + p;
	const uint32_t flg = src[3];                                             // (a candidate: p + 4 <= nbytes)
	uint32_t at = 10;
	bool ok = at < n;
	if (ok && (flg & 4)) {                                                   // FEXTRA
		ok = n >= 12;
		if (ok) {
			at = 12 + index_rd16(src + 10);
			ok = at < n;
		}
	}
	if (ok && (flg & 8)) {                                                   // FNAME
		at = frame_skip_cstring(src, at, n, lane);
		ok = at < n;
	}
	if (ok && (flg & 16)) {                                                  // FCOMMENT
		at = frame_skip_cstring(src, at, n, lane);
		ok = at < n;
	}
	if (ok && (flg & 2)) {                                                   // FHCRC: skipped, not verified
		at += 2;
		ok = at < n;
	}
	if (lane == 0) {
		hdr[row] = ok ? at : 0u;
		status[row] = ok ? HD_OK : PIECE_CUT;
	}
}

// step 2, one lane per candidate: the sized candidates get their class -- what ran out of the window is CUT where the
// window ends at nbytes and LONG where max_in ended it; a stream of 2^32 bytes or more is no member -- and every member's
// end is resolved to a candidate, as k_index_links does.  The head of the chain is the candidate at lo.
__global__ __launch_bounds__(256) void k_any_links(uint64_t nbytes, uint64_t lo, uint32_t max_in, const uint64_t *pos, uint32_t ncand,
						    const uint32_t *tosize, const int32_t *pstat, uint32_t *cls, const uint32_t *total,
						    uint32_t *succ, uint32_t *mark)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	const uint64_t p = pos[i];
	uint32_t c = cls[i];
	if (tosize[i]) {
		const int32_t st = pstat[i];
		c = st == HD_OK ? MEMBER_OK : st != PIECE_CUT ? MEMBER_BAD : nbytes - p <= max_in ? MEMBER_CUT : MEMBER_LONG;
		cls[i] = c;
	}
	uint32_t s = IDX_NIL;
	if (c == MEMBER_OK) {
		const uint64_t next = p + total[i];
		uint32_t l = i + 1, h = ncand;
		while (l < h) {
			const uint32_t mid = l + ((h - l) >> 1);
			if (pos[mid] < next)
				l = mid + 1;
			else
				h = mid;
		}
		if (l < ncand && pos[l] == next)
			s = l;
	}
	succ[i] = s;
	mark[i] = i == 0 && p == lo && c == MEMBER_OK;
}

// k_members_tables with offsets from `base` on (pos[] counts from there) and out_size from the decode where there was one
__global__ __launch_bounds__(256) void k_any_tables(const uint8_t *blob, uint64_t base, const uint64_t *pos, const uint32_t *hdr,
						     const uint32_t *total, const uint32_t *osize, const uint32_t *tosize, const uint32_t *mark,
						     const uint64_t *rank, uint32_t ncand, uint64_t nrows, uint32_t max_members, uint64_t *in_off,
						     uint32_t *in_len, uint32_t *out_size, uint32_t *crc_want, uint64_t *end_offset)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i], p = pos[i];
	const uint32_t h = hdr[i], t = total[i];
	if (r < max_members) {
		in_off[r] = base + p + h;
		in_len[r] = t - h;
		crc_want[r] = index_rd32(blob + p + t - 8);
		out_size[r] = tosize[i] ? osize[i] : index_rd32(blob + p + t - 4);
	}
	if (r + 1 == nrows)
		*end_offset = p + t;
}

// sum[] = { nmembers, out_bytes, end_offset, status }.  The stop position's verdict is its candidate's class; a position
// that is no candidate is BAD, or CUT where fewer than four bytes are left and the magic fits as far as they go.
__global__ void k_any_verdict(const uint8_t *blob, uint64_t nbytes, uint64_t base, uint64_t lo, const uint64_t *pos, const uint32_t *cls,
			      uint32_t ncand, uint64_t nrows, uint32_t max_members, uint64_t *sum)
{
	const uint64_t end = nrows ? sum[2] : lo;
	uint64_t status = 0;
	if (end < nbytes) {
		uint32_t l = 0, h = ncand;
		while (l < h) {
			const uint32_t mid = l + ((h - l) >> 1);
			if (pos[mid] < end)
				l = mid + 1;
			else
				h = mid;
		}
		if (l < ncand && pos[l] == end) {
			status = cls[l];
		} else {
			const uint64_t avail = nbytes - end;
			const uint8_t *b = blob + end;
			const bool fits = avail < 4 && b[0] == 0x1f && (avail < 2 || b[1] == 0x8b) && (avail < 3 || b[2] == 8);
			status = fits ? MEMBER_CUT : MEMBER_BAD;
		}
	}
	if (nrows > max_members)
		status = 3;
	sum[0] = nrows;
	sum[2] = base + end;
	sum[3] = status;
}

} // namespace hd
