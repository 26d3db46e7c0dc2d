// hd_inflate_common.hpp -- what the three DEFLATE decoders of the device share: everything that READS a stream.
//
// hd_inflate.hpp (throughput, one wavefront per stream), hd_inflate_lat.hpp (latency, four wavefronts per stream) and
// hd_inflate_size.hpp (the size pass and the piece decoder: no output at all) differ in what they do with a token -- the
// ring, window placement, the pipe between wavefronts, the flush, the CRC: that stays with each of them.  How a token is
// FOUND is one thing, and it is here once: the entry formats and the table builder, the bit reader, the block headers,
// a lane's speculative decode and the scalar walk over a window.  (Not the scalar path's checked decode of one token: each
// decoder keeps its copy, a shared function was slower in all three -- DESIGN.md 4.3c.)  Accept/reject behaviour follows
// libdeflate; oracle/hd_inflate.c lists the rules with their file:line.
#pragma once
#include <type_traits>
#include "hd_device.hpp"

namespace hd {

#ifdef HD_INFLATE_STATS
// experiment build only (tools/exp_inflate_stats.sh): where the tokens go
__device__ unsigned long long g_inf_stats[8];
__device__ unsigned long long g_inf_stats2[8];      // matches of the windows: [0] all [1] lane groups of 8 [2] of 16 [3] simple, one at a time [4] far, one at a time [5] general (fed by the window, overlapping, > 64 bytes)
#define INF_STAT2(k, v) atomicAdd(&g_inf_stats2[k], lane == 0 ? (unsigned long long)(v) : 0ull)
#define INF_U64(m) (((uint64_t)uniform((uint32_t)((m) >> 32)) << 32) | uniform((uint32_t)(m)))
__device__ unsigned long long g_inf_cycles[8];       // [0] block headers + table build, [1] windows, [2] scalar token path, [3] whole kernel
// (every lane adds, lane 0 the value and the others zero: an `if (lane == 0)` around the atomic makes the compiler treat the
// lane masks that live across it as divergent, and the window code keeps them in scalar registers)
#define INF_STAT(k, v) atomicAdd(&g_inf_stats[k], lane == 0 ? (unsigned long long)(v) : 0ull)
#define INF_T0(t) const unsigned long long t = __builtin_amdgcn_s_memtime()
// (cycles are summed in scalar registers and leave once per wave)
#define INF_T1(k, t) do { inf_cyc[k] += __builtin_amdgcn_s_memtime() - (t); } while (0)
#define INF_CYC_DECL unsigned long long inf_cyc[4] = { 0, 0, 0, 0 }
#define INF_CYC_FLUSH do { for (int k_ = 0; k_ < 4; k_++) atomicAdd(&g_inf_cycles[k_], lane == 0 ? inf_cyc[k_] : 0ull); } while (0)
#else
#define INF_STAT(k, v) do { } while (0)
#define INF_STAT2(k, v) do { } while (0)
#define INF_T0(t) do { } while (0)
#define INF_T1(k, t) do { } while (0)
#define INF_CYC_DECL do { } while (0)
#define INF_CYC_FLUSH do { } while (0)
#endif

constexpr uint32_t INF_LT_BITS = 9;      // litlen direct table (8 VGPRs once loaded)
constexpr uint32_t INF_DT_BITS = 8;      // offset direct table

// table entry: [31:16] value (literal / length base / offset base)
//              [9:8] kind  [7:4] extra-bit count  [3:0] codeword length
constexpr uint32_t K_LIT = 0, K_LEN = 1, K_EOB = 2, K_SLOW = 3;

// order in which the precode lengths are stored (RFC 1951 3.2.7;
// decompress_template.h:91-93)
__constant__ uint8_t k_precode_perm[19] = { 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 };

__device__ __forceinline__ uint32_t litlen_entry(uint32_t sym, uint32_t len)
{
	if (sym < 256)
		return (sym << 16) | (K_LIT << 8) | len;
	if (sym == 256)
		return (K_EOB << 8) | len;
	// lengths: deflate_decompress.c:563-577 (286, 287 decode as 258)
	uint32_t s = sym - 257, base, eb;
	if (s < 8) { base = 3 + s; eb = 0; }
	else if (s >= 28) { base = 258; eb = 0; }
	else { eb = (s >> 2) - 1; base = 3 + ((4 + (s & 3)) << eb); }
	return (base << 16) | (K_LEN << 8) | (eb << 4) | len;
}

__device__ __forceinline__ uint32_t offset_entry(uint32_t sym, uint32_t len)
{
	// deflate_decompress.c:612-627 (30, 31 decode as 24577 + 13 bits)
	uint32_t base, eb;
	if (sym < 4) { base = 1 + sym; eb = 0; }
	else if (sym >= 30) { base = 24577; eb = 13; }
	else { eb = (sym >> 1) - 1; base = 1 + ((2 + (sym & 1)) << eb); }
	return (base << 16) | (eb << 4) | len;
}

constexpr uint32_t INF_T_SCRATCH = 320;      // byte offset in cl of { u32 cnt[16]; u16 first[16]; u16 offs[16]; }

// Build one decode table from code lengths (all 64 lanes).  Returns false for
// what build_decode_table() rejects (deflate_decompress.c:799-853).
//   nsyms <= 288; tbits = direct table bits; kind 0 litlen / 1 offset / 2 precode
// Per-length counters live in LDS (one lane per code length), not in registers:
// sixteen-element uniform arrays would cost 64 SGPRs and spill the symbol loop.
template <int KIND>
__device__ __noinline__ uint32_t build_table(const uint8_t *lens, uint32_t nsyms, uint32_t *table, uint32_t tbits,
					  uint16_t *sorted, uint16_t *count_out, uint8_t *scratch, uint32_t lane)
{
	// per-length counters; once the counts are read they serve as the running rank bases
	uint32_t *t_cnt = (uint32_t *)scratch, *t_base = t_cnt;
	uint16_t *t_first = (uint16_t *)(scratch + 64), *t_offs = t_first + 16;
	if (lane < 16)
		t_cnt[lane] = 0;
	for (uint32_t base = 0; base < nsyms; base += 64) {
		const uint32_t s = base + lane;
		const uint32_t len = s < nsyms ? lens[s] : 0;
		if (len)
			atomicAdd(&t_cnt[len], 1u);
	}
	// lane l (1..15) derives its length's first codeword, sorted offset and codespace share
	uint32_t code = 0, o = 0, mine = 0;
	if (lane >= 1 && lane < 16) {
		for (uint32_t l = 1; l <= lane; l++) {
			code = (code + (l > 1 ? t_cnt[l - 1] : 0)) << 1;
			if (l < lane)
				o += t_cnt[l];
		}
		mine = t_cnt[lane];
		t_first[lane] = (uint16_t)code;       // < 2^15 for every code that passes the checks below
		t_offs[lane] = (uint16_t)o;
	}
	if (lane < 16)
		t_base[lane] = 0;                     // (all lanes are past the loop that read the counts)
	if (count_out && lane < 16)
		count_out[lane] = (uint16_t)mine;
	const uint32_t used = readlane(wave_incl_scan((lane >= 1 && lane < 16) ? mine << (15 - lane) : 0u), 63);
	const uint64_t present = __ballot(mine != 0);
	const uint32_t maxlen = present ? 63 - (uint32_t)__clzll((long long)present) : 0;
	const uint32_t ones = readlane(mine, 1);
	if (used > (1u << 15))
		return 0;                         // overfull
	bool degenerate = false;
	if (used < (1u << 15)) {                  // incomplete
		if (used != 0 && !(ones == 1 && maxlen == 1))
			return 0;
		degenerate = true;
	}
	uint32_t one_sym = 0;                 // the symbol owning the single 1-bit codeword, if any
	for (uint32_t base = 0; base < nsyms; base += 64) {
		const uint32_t s = base + lane;
		const uint32_t len = s < nsyms ? lens[s] : 0;
		// rank inside the length class, in symbol order: one ballot per length present
		uint32_t rank = 0;
		uint64_t rem = __ballot(len != 0);
		while (rem) {
			const uint32_t lead = (uint32_t)__ffsll((unsigned long long)rem) - 1;
			const uint32_t lc = readlane(len, lead);
			const uint64_t m = __ballot(len == lc);
			const uint32_t b0 = uniform(t_base[lc]);
			if (len == lc)
				rank = b0 + __popcll(m & ((1ull << lane) - 1));
			if (lane == lead)
				t_base[lc] = b0 + __popcll(m);
			if (lc == 1)
				one_sym = base + lead;
			rem &= ~m;
		}
		if (len) {
			sorted[t_offs[len] + rank] = (uint16_t)s;
			const uint32_t cw = t_first[len] + rank;        // MSB-first codeword
			const uint32_t rev = __brev(cw) >> (32 - len);
			if (!degenerate) {
				if (len <= tbits) {
					const uint32_t e = KIND == 0 ? litlen_entry(s, len)
							 : KIND == 1 ? offset_entry(s, len)
								     : ((s << 16) | len);
					for (uint32_t i = rev; i < (1u << tbits); i += 1u << len)
						table[i] = e;
				} else {
					table[rev & ((1u << tbits) - 1)] = K_SLOW << 8;
				}
			}
		}
	}
	if (degenerate) {
		// empty code -> symbol 0; single 1-bit codeword -> that symbol, for both
		// bit values (deflate_decompress.c:816-849)
		const uint32_t sym = used ? one_sym : 0;
		const uint32_t e = KIND == 0 ? litlen_entry(sym, 1) : KIND == 1 ? offset_entry(sym, 1) : ((sym << 16) | 1);
		for (uint32_t i = lane; i < (1u << tbits); i += 64)
			table[i] = e;
	}
	return 1;
}

// Canonical decode for codewords longer than the direct table; returns symbol | length << 16.
// All fifteen lengths are tried at once: lane l holds count[l], two prefix sums give its length's first
// codeword (first[l] = sum_{k<l} count[k] << (l - k), i.e. the Kraft sum in 2^-15 units shifted back) and
// its offset into the sorted symbols, one ballot finds the length that matches.  (The bit-serial loop it
// replaces paid an LDS round trip per length: ~1 M such tokens per GiB of a libdeflate-6 stream.)
__device__ __noinline__ uint32_t slow_decode(uint64_t bb, const uint16_t *count, const uint16_t *sorted, uint32_t lane)
{
	const bool in = lane >= 1 && lane < 16;
	const uint32_t l = lane & 15;
	const uint32_t cnt = in ? count[l] : 0u;
	const uint32_t scaled = cnt << (15 - l);
	const uint32_t first = (wave_incl_scan(scaled) - scaled) >> (15 - l);
	const uint32_t offs = wave_incl_scan(cnt) - cnt;
	const uint32_t code = __brev((uint32_t)bb) >> (32 - (l ? l : 1));     // the first l stream bits, MSB first
	const uint32_t d = code - first;
	const uint64_t hit = __ballot(in && d < cnt);
	if (!hit)
		return 15u << 16;
	const uint32_t len = (uint32_t)__ffsll((unsigned long long)hit) - 1;
	return (uint32_t)sorted[readlane(offs + d, len)] | (len << 16);
}

// ---- the bit reader --------------------------------------------------------------------------------------------------
// The compressed stream is pulled in 256-byte coalesced pieces, one dword per lane (cw holds piece cur_piece, cw_next the
// one behind it, requested a piece ahead of its use); the bit buffer is uniform and lives in scalar registers, refilled a
// dword at a time with v_readlane.  Positions are 32-bit BIT counts from src32, the stream's first aligned dword: the
// callers refuse a stream of HD_INFLATE_MAX_IN bytes or more.  Bits behind the stream's last byte read as 0.
struct InfReader {
	const uint32_t *src32;
	uint32_t nbytes_al;              // valid bytes from src32
	uint32_t mis;                    // bytes between src32 and the stream
	uint32_t lane;
	uint32_t over_t;                 // consumed_bits() > 8 n + 64 in 32-bit arithmetic (n < 2^28): (dw << 5) - bc > over_t
	uint32_t cur_piece, cw, cw_next;
	uint32_t dw;                     // next dword index to feed the bit buffer
	uint64_t bb;                     // bit buffer (uniform)
	uint32_t bc;                     // valid bits in bb

	__device__ __forceinline__ InfReader(const uint8_t *src, uint32_t n, uint32_t lane_)
		: src32((const uint32_t *)(src - ((uintptr_t)src & 3))), nbytes_al((uint32_t)((uintptr_t)src & 3) + n),
		  mis((uint32_t)((uintptr_t)src & 3)), lane(lane_), over_t(8 * n + 64 + 8 * mis), cur_piece(0), dw(0), bb(0), bc(0)
	{
		cw = load_piece(0);
		cw_next = load_piece(1);
		// skip the mis-alignment bytes
		refill();
		bb >>= 8 * mis;
		bc -= 8 * mis;
	}
	__device__ __forceinline__ uint32_t load_piece(uint32_t piece) const
	{
		const uint32_t d = piece * 64 + lane;
		uint32_t w = 0;
		if (d * 4 < nbytes_al) {
			w = src32[d];
			const uint32_t valid = nbytes_al - d * 4;    // bytes of this dword inside the stream
			if (valid < 4)
				w &= (1u << (8 * valid)) - 1;
		}
		return w;
	}
	__device__ __forceinline__ void refill()
	{
		if (bc <= 32) {
			const uint32_t piece = dw >> 6;
			if (piece != cur_piece) {        // uniform branch: step to the next piece
				cw = cw_next;
				cur_piece = piece;
				cw_next = load_piece(piece + 1);
			}
			bb |= (uint64_t)readlane(cw, dw & 63) << bc;
			dw++;
			bc += 32;
		}
	}
	__device__ __forceinline__ void drop(uint32_t nbits)
	{
		bb >>= nbits;
		bc -= nbits;
	}
	__device__ __forceinline__ int64_t consumed_bits() const { return (int64_t)dw * 32 - bc - 8 * (int64_t)mis; }
	__device__ __forceinline__ bool overrun() const { return (dw << 5) - bc > over_t; }
	__device__ __forceinline__ uint32_t bit_pos() const { return (dw << 5) - bc; }      // from src32: what seek_bit takes
	__device__ __forceinline__ void seek_bit(uint32_t B)                               // restart at bit B from src32
	{
		dw = B >> 5;
		const uint32_t piece = dw >> 6;
		if (piece != cur_piece) {
			if (piece == cur_piece + 1)
				cw = cw_next;
			else
				cw = load_piece(piece);
			cur_piece = piece;
			cw_next = load_piece(piece + 1);
		}
		bb = 0;
		bc = 0;
		refill();
		drop(B & 31);
	}
	__device__ __forceinline__ void seek_byte(uint32_t byteoff) { seek_bit(8 * (mis + byteoff)); }   // ... at src + byteoff
};

// ---- block headers ---------------------------------------------------------------------------------------------------
// LDS is any of the decoders' layouts: lit / off (the direct tables), lit_sorted / off_sorted / lit_count / off_count (the
// slow path's), cl / pre_lens (the code lengths, live only here; the table builder's scratch at cl + INF_T_SCRATCH).

// A dynamic block's header (decompress_template.h:101-232): HLIT / HDIST / HCLEN, the precode, the run-length coded code
// lengths, the two tables.  n = the stream's bytes.  False for what libdeflate rejects: the caller answers HD_BAD_DATA.
template <class LDS>
__device__ __forceinline__ bool inflate_dynamic_header(InfReader &R, LDS &L, uint32_t n, uint32_t lane)
{
	R.refill();
	const uint32_t nlit = 257 + ((uint32_t)R.bb & 31);
	const uint32_t noff = 1 + (((uint32_t)R.bb >> 5) & 31);
	const uint32_t npre = 4 + (((uint32_t)R.bb >> 10) & 15);
	R.drop(14);
	if (lane < 19)
		L.pre_lens[lane] = 0;
	for (uint32_t i = 0; i < npre; i++) {
		R.refill();
		if (lane == 0)
			L.pre_lens[k_precode_perm[i]] = (uint8_t)((uint32_t)R.bb & 7);
		R.drop(3);
	}
	if (!uniform(build_table<2>(L.pre_lens, 19, L.lit, 7, L.lit_sorted, nullptr, L.cl + INF_T_SCRATCH, lane)))
		return false;
	uint8_t *cl = L.cl;
	uint32_t i = 0, prev = 0;
	while (i < nlit + noff) {
		R.refill();
		if (R.consumed_bits() > 8 * (int64_t)n + 64)
			return false;
		const uint32_t e = uniform(L.lit[(uint32_t)R.bb & 127]);
		const uint32_t s = e >> 16;
		R.drop(e & 15);
		if (s < 16) {
			if (lane == 0)
				cl[i] = (uint8_t)s;
			prev = s;
			i++;
			continue;
		}
		uint32_t rep, val = 0;
		if (s == 16) {
			if (i == 0)
				return false;
			rep = 3 + ((uint32_t)R.bb & 3);
			R.drop(2);
			val = prev;
		} else if (s == 17) {
			rep = 3 + ((uint32_t)R.bb & 7);
			R.drop(3);
			prev = 0;
		} else {
			rep = 11 + ((uint32_t)R.bb & 127);
			R.drop(7);
			prev = 0;
		}
		for (uint32_t k = lane; k < rep; k += 64)
			cl[i + k] = (uint8_t)val;
		i += rep;
	}
	if (i != nlit + noff)
		return false;
	return uniform(build_table<1>(cl + nlit, noff, L.off, INF_DT_BITS, L.off_sorted, L.off_count, L.cl + INF_T_SCRATCH, lane)) &&
	       uniform(build_table<0>(cl, nlit, L.lit, INF_LT_BITS, L.lit_sorted, L.lit_count, L.cl + INF_T_SCRATCH, lane));
}

// the static codes' tables (decompress_template.h:297-330)
template <class LDS>
__device__ __forceinline__ void inflate_static_tables(LDS &L, uint32_t lane)
{
	uint8_t *cl = L.cl;
	for (uint32_t s = lane; s < 320; s += 64)
		cl[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
	build_table<1>(cl + 288, 32, L.off, INF_DT_BITS, L.off_sorted, L.off_count, L.cl + INF_T_SCRATCH, lane);
	build_table<0>(cl, 288, L.lit, INF_LT_BITS, L.lit_sorted, L.lit_count, L.cl + INF_T_SCRATCH, lane);
}

// ---- the window decode: what FINDS the tokens --------------------------------------------------------------------------
// A window is 128 bits of the stream.  Every lane decodes the token that WOULD start at its bit offset (two LDS table
// gathers, vector instructions only); a short scalar walk then follows the real chain from the window's first bit.
struct InfSpec {
	uint32_t e;                      // the litlen entry (a literal's byte in [31:16])
	uint32_t length, offset;         // a match's; length is a literal's byte where the token is one
	uint32_t outlen;                 // bytes the token puts out: 1, the length, 0 (end of block, long codeword)
	uint32_t walk;                   // the token's bits | 64 where the walk stops in front of it
	uint64_t is_len, is_lit;         // lane masks (one v_cmp each, used through sel())
};
// the token at bit bl of the three dwords lo, mid, hi (only bl & 31 counts)
template <class LDS>
__device__ __forceinline__ InfSpec spec_token(const LDS &L, uint32_t bl, uint32_t lo, uint32_t mid, uint32_t hi)
{
	InfSpec r;
	const uint32_t a = __builtin_amdgcn_alignbit(mid, lo, bl & 31);
	const uint32_t bq = __builtin_amdgcn_alignbit(hi, mid, bl & 31);
	const uint32_t e = L.lit[a & ((1u << INF_LT_BITS) - 1)];
	const uint32_t len1 = e & 15, eb = (e >> 4) & 15;
	r.e = e;
	r.length = (e >> 16) + __builtin_amdgcn_ubfe(a, len1, eb);         // (one v_bfe_u32; width 0 gives 0)
	const uint32_t t1 = len1 + eb;                 // <= 9 + 5
	const uint32_t rest = __builtin_amdgcn_alignbit(bq, a, t1);
	const uint32_t dd = L.off[rest & ((1u << INF_DT_BITS) - 1)];
	const uint32_t kind2 = e & 0x300;
	r.is_len = __ballot(kind2 == (K_LEN << 8));
	r.is_lit = __ballot(kind2 == (K_LIT << 8));
	// (the offset entry counts for a length only: masked here, its fields are zero elsewhere -- and so is
	// eb in a literal's or an end-of-block's entry, so the token's bits are one sum)
	const uint32_t ddm = sel(r.is_len, dd, 0u);
	const uint32_t dlen = ddm & 15, deb = (ddm >> 4) & 15;
	r.offset = (ddm >> 16) + __builtin_amdgcn_ubfe(rest, dlen, deb);
	const uint32_t tokbits = t1 + dlen + deb;
	r.outlen = sel(r.is_lit, 1u, sel(r.is_len, r.length, 0u));
	// bit 6 = the walk stops in front of this token: bit 9 of either entry (K_EOB and K_SLOW have it)
	// moved down.  (A zero-bit token cannot come out of a well-formed table; the max keeps the walk
	// moving whatever the table holds.)
	const uint32_t tb1 = tokbits ? tokbits : 1u;
	r.walk = tb1 | ((e >> 3) & 64u) | ((ddm >> 3) & 64u);
	return r;
}

// The real chain from bit 0 of the window, over the walk words of its two halves (lane = bit position).  This walk is
// the hottest scalar code of the decoders (the CU has one scalar ALU) and the compiler spends ~20 instructions per token
// on it, so it is written out: 3 SALU + 1 branch + 1 v_readlane per token (the lane select of v_readlane and s_bitset1
// take the low 6 bits, so the second half runs on the position itself).  It stops in front of the first token a window
// cannot take; that one goes to the scalar path.  The stop flag is bit 6 of the word that is ADDED to the position, so
// such a token throws the walk out of its half by itself and is taken back behind the loop.  (Testing the flag before
// every add, seven instructions and two branches, measured 1.0-1.3 % less throughput: profiles/r05_inflate_cuts.txt.)
// (A lane select written by the SALU needs no wait states before v_readlane, only one written by the VALU does.)
// Out: bits = the window's bits the real tokens take, real0 / real1 = lane masks of the bits of each half at which a real
// token starts, last = the last word read (& 64: the walk stopped in front of its token).
__device__ __forceinline__ void window_walk(uint32_t walk0, uint32_t walk1, uint32_t &bits, uint64_t &real0, uint64_t &real1, uint32_t &last)
{
	asm volatile("s_mov_b32 %0, 0\n\t"
		     "s_mov_b64 %1, 0\n\t"
		     "s_mov_b64 %2, 0\n"
		     "Lhd_walk0_%=:\n\t"
		     "v_readlane_b32 %3, %4, %0\n\t"
		     "s_bitset1_b64 %1, %0\n\t"
		     "s_add_u32 %0, %0, %3\n\t"
		     "s_cmp_lt_u32 %0, 64\n\t"
		     "s_cbranch_scc1 Lhd_walk0_%=\n\t"
		     "s_bitcmp1_b32 %3, 6\n\t"
		     "s_cbranch_scc0 Lhd_walk1_%=\n\t"
		     "s_sub_u32 %0, %0, %3\n\t"
		     "s_bitset0_b64 %1, %0\n\t"
		     "s_branch Lhd_walk_done_%=\n"
		     "Lhd_walk1_%=:\n\t"
		     "v_readlane_b32 %3, %5, %0\n\t"
		     "s_bitset1_b64 %2, %0\n\t"
		     "s_add_u32 %0, %0, %3\n\t"
		     "s_cmp_lt_u32 %0, 128\n\t"
		     "s_cbranch_scc1 Lhd_walk1_%=\n\t"
		     "s_bitcmp1_b32 %3, 6\n\t"
		     "s_cbranch_scc0 Lhd_walk_done_%=\n\t"
		     "s_sub_u32 %0, %0, %3\n\t"
		     "s_bitset0_b64 %2, %0\n"
		     "Lhd_walk_done_%=:"
		     : "=&s"(bits), "=&s"(real0), "=&s"(real1), "=&s"(last)
		     : "v"(walk0), "v"(walk1)
		     : "scc");
}

} // namespace hd
