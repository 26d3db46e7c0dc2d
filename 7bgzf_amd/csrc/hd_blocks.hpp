// hd_blocks.hpp -- a plain DEFLATE stream, which has NO flush point, decoded in parallel rows.
//
// Role: the reader of applet/7gzip.c:8-116 and zlibrawstdio, and zlib's inflate() on what gzip, zlib.compress or a gzip
// writer of libdeflate put out: one serial decode.  hd_stream.hpp and hd_carry.hpp find the byte-aligned markers a flush
// leaves; such a stream has none, and both answer "one row".  What it has is BLOCKS, which start at any bit.  This is
// hd_stream.hpp's index once more, with a header rule in the place of the 00 00 ff ff marker and bit positions in the place
// of byte positions, and hd_carry.hpp's marker path behind it, since every block reaches back into the one in front:
//   index   k_blocks_flag / k_blocks_write   one streaming read finds every BIT at which a non-final dynamic block header
//                                  could start (block_header_rule); with the first payload bit they are the candidates
//           k_blocks_piece         hd_inflate_size.hpp's piece decoder in its carried form, started on a bit: block after
//                                  block to the end of a final block (PIECE_FINAL) or to a block end with BFINAL 0 / BTYPE 2
//                                  behind it (PIECE_NEXT); in_used in BITS
//           k_blocks_count         (the bench's) how many pieces got past their first header, how many decode
//           k_blocks_links         a NEXT piece links to the candidate at its end bit; k_index_jump and the prefix count
//                                  mark and rank the chain from candidate 0, as they stand
//           k_blocks_sizes .. k_blocks_reach   the chain's pieces merged into rows of about row_bytes of output: the row
//                                  of a piece by a prefix count of the pieces that begin one, the row's reach a segmented
//                                  maximum over its pieces
//           k_blocks_verdict       where the chain stopped and why
//   decode  k_blocks_check_rows    a caller's table held to the rules of bit rows
//           k_blocks_decode        k_carry_decode started on bit in_off & 7, ended on bit in_len
//           and hd_carry.hpp's tails, resolve, verify and check, unchanged.
// Every read of the stream is bounded by the payload's end, whatever the stream says; no kernel waits for another.
#pragma once
#include "hd_carry.hpp"

namespace hd {

constexpr uint32_t BLOCK_HDR_NO = 0, BLOCK_HDR_YES = 1, BLOCK_HDR_SHORT = 2;

// ---- the header rule ---------------------------------------------------------------------------------------------------
// Could a non-final dynamic block header start here?  v0 | v1: the 96 stream bits from some byte, k < 8 the bit in it, left
// the bits from that position to the payload's end.  The bits must read BFINAL 0, BTYPE 2, HLIT (5), HDIST (5), HCLEN (4),
// then HCLEN + 4 precode lengths of 3 bits, all in front of the payload's end (else: SHORT), and the precode must be one
// build_table<2> (hd_inflate_common.hpp) takes: with K = the sum of 2^(7 - len) over the non-zero lengths, K == 128
// (complete), K == 0 (empty), or one non-zero length that is 1.  Nothing else is examined -- inflate_dynamic_header puts
// no bound on HLIT / HDIST -- so the rule is a NECESSARY condition of that function accepting: it drops no header the
// decoder would take.  On random bits it passes 5.13e-4 of the positions, one per 244 bytes of stream.
__device__ __forceinline__ uint32_t block_header_rule(uint64_t v0, uint32_t v1, uint32_t k, uint64_t left)
{
	if (left < 3)
		return BLOCK_HDR_SHORT;
	const uint32_t x = (uint32_t)(v0 >> k);
	if ((x & 7) != 4)
		return BLOCK_HDR_NO;
	if (left < 17)
		return BLOCK_HDR_SHORT;
	const uint32_t npre = 4 + ((x >> 13) & 15);
	if (left < 17 + 3 * npre)
		return BLOCK_HDR_SHORT;
	uint64_t y = (v0 >> (k + 17)) | ((uint64_t)v1 << (47 - k));      // the 57 bits behind HCLEN
	y &= (1ull << (3 * npre)) - 1;
	uint32_t K = 0, nz = 0;
#pragma unroll
	for (uint32_t i = 0; i < 19; i++) {
		const uint32_t l = (uint32_t)(y >> (3 * i)) & 7;
		K += l ? 128u >> l : 0u;
		nz += l != 0;
	}
	return (K == 128 || K == 0 || (K == 64 && nz == 1)) ? BLOCK_HDR_YES : BLOCK_HDR_NO;
}

// the rule at bit p of a stream of `end` bytes, the bytes fetched one by one (the verdict, the test entry)
__device__ inline uint32_t block_header_at(const uint8_t *strm, uint64_t end, uint64_t p)
{
	if (p >= 8 * end)
		return BLOCK_HDR_SHORT;
	const uint64_t o = p >> 3;
	uint64_t v0 = 0;
	uint32_t v1 = 0;
	for (uint32_t j = 0; j < 8; j++)
		v0 |= (uint64_t)(o + j < end ? strm[o + j] : 0) << (8 * j);
	for (uint32_t j = 0; j < 4; j++)
		v1 |= (uint32_t)(o + 8 + j < end ? strm[o + 8 + j] : 0) << (8 * j);
	return block_header_rule(v0, v1, (uint32_t)p & 7, 8 * end - p);
}

// the test entry's kernel: one lane per position
__global__ __launch_bounds__(256) void k_blocks_rule(const uint8_t *strm, uint64_t end, const uint64_t *pos, uint32_t n, uint32_t *verdict)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n)
		verdict[i] = block_header_at(strm, end, pos[i]);
}

// ---- the candidates: hd_index.hpp's two passes (index_flag_body's words and bitmap) over bit positions ------------------------
// The 128 bit positions of the 16 bytes at o (a multiple of 16): bit 8 j + k of lo | hi << 64 is set where position
// 8 (o + j) + k passes the rule and lies in [lo_bit, 8 end).  A header is at most 74 bits, so with k <= 7 the twelve bytes
// from o + j hold it: seven dwords from o, moved on a byte at a time.  Bytes at and behind `end` read as 0 and are never
// examined.
__device__ __forceinline__ void blocks_granule(const uint8_t *strm, uint64_t end, uint64_t o, uint64_t lo_bit, uint64_t &lo, uint64_t &hi)
{
	lo = hi = 0;
	if (8 * (o + 16) <= lo_bit || o >= end)
		return;
	uint32_t d[7];
	if (o + 28 <= end) {
		const uint4 v = *(const uint4 *)(strm + o);
		const uint32_t *q = (const uint32_t *)(strm + o + 16);
		d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
		d[4] = q[0], d[5] = q[1], d[6] = q[2];
	} else {
#pragma unroll
		for (uint32_t k = 0; k < 7; k++)
			d[k] = 0;
#pragma unroll
		for (uint32_t k = 0; k < 28; k++)
			d[k >> 2] |= (o + k < end ? (uint32_t)strm[o + k] : 0u) << (8 * (k & 3));
	}
	const uint64_t end_bit = 8 * end;
#pragma unroll 1
	for (uint32_t j = 0; j < 16; j++) {
		const uint64_t v0 = (uint64_t)d[0] | (uint64_t)d[1] << 32, p0 = 8 * (o + j);
		uint32_t m = 0;
		if (p0 < end_bit)
#pragma unroll 1
			for (uint32_t k = 0; k < 8; k++)
				if (p0 + k >= lo_bit && block_header_rule(v0, d[2], k, end_bit - p0 - k) == BLOCK_HDR_YES)
					m |= 1u << k;
		if (j < 8)
			lo |= (uint64_t)m << (8 * j);
		else
			hi |= (uint64_t)m << (8 * (j - 8));
#pragma unroll
		for (uint32_t k = 0; k < 6; k++)
			d[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], 1);
		d[6] >>= 8;
	}
}

// A tile of the two passes is BLOCK_TILE_WORDS bitmap words and ONE wavefront, so that neither pass needs LDS: the tile's
// count is one wavefront's sum, and the write pass's order inside a tile is one wavefront's prefix sum.
constexpr uint32_t BLOCK_TILE_WORDS = 64;

// pass 1: per 1 KiB word a ballot of the granules that hold a candidate, per tile the candidate count
__global__ __launch_bounds__(64) void k_blocks_flag(const uint8_t *strm, uint64_t end, uint64_t lo_bit, uint64_t *bitmap, uint32_t *tile_cnt)
{
	const uint32_t lane = threadIdx.x;
	const uint64_t word0 = (uint64_t)blockIdx.x * BLOCK_TILE_WORDS;
	uint32_t cnt = 0;
	for (uint32_t it = 0; it < BLOCK_TILE_WORDS; it++) {
		const uint64_t base = (word0 + it) * IDX_WORD;
		if (base >= end)
			break;
		uint64_t lo, hi;
		blocks_granule(strm, end, base + lane * 16, lo_bit, lo, hi);
		cnt += __popcll(lo) + __popcll(hi);
		const uint64_t any = __ballot((lo | hi) != 0);
		if (lane == 0)
			bitmap[word0 + it] = any;
	}
	for (int o = 32; o > 0; o >>= 1)
		cnt += (uint32_t)__shfl_down((int)cnt, o, 64);
	if (lane == 0)
		tile_cnt[blockIdx.x] = cnt;
}

// pass 2: lane t of tile b owns bitmap word b * 64 + t; it judges the flagged granules again, and the candidates of the
// tile go to pos[tile_off[b]...] in ascending order, as BIT positions
__global__ __launch_bounds__(64) void k_blocks_write(const uint8_t *strm, uint64_t end, uint64_t lo_bit, const uint64_t *bitmap,
						      uint64_t nwords, const uint64_t *tile_off, uint64_t *pos)
{
	const uint64_t wi = (uint64_t)blockIdx.x * BLOCK_TILE_WORDS + threadIdx.x;
	const uint64_t bits = wi < nwords ? bitmap[wi] : 0;
	uint32_t c = 0;
	for (uint64_t b = bits; b; b &= b - 1) {
		uint64_t lo, hi;
		blocks_granule(strm, end, wi * IDX_WORD + (uint32_t)__ffsll((long long)b) * 16 - 16, lo_bit, lo, hi);
		c += __popcll(lo) + __popcll(hi);
	}
	uint64_t at = tile_off[blockIdx.x] + (wave_incl_scan(c) - c);
	for (uint64_t b = bits; b; b &= b - 1) {
		const uint64_t o = wi * IDX_WORD + (uint32_t)__ffsll((long long)b) * 16 - 16;
		uint64_t lo, hi;
		blocks_granule(strm, end, o, lo_bit, lo, hi);
		for (; lo; lo &= lo - 1)
			pos[at++] = 8 * o + (uint32_t)__ffsll((long long)lo) - 1;
		for (; hi; hi &= hi - 1)
			pos[at++] = 8 * o + 64 + (uint32_t)__ffsll((long long)hi) - 1;
	}
}

// one lane per candidate: how many pieces got past their own first block header (stop != 0), how many decode to their stop
__global__ __launch_bounds__(256) void k_blocks_count(const uint32_t *stop, const uint32_t *in_used, uint32_t ncand, unsigned long long *out2)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	const uint64_t past = __ballot(i < ncand && stop[i] != 0), whole = __ballot(i < ncand && in_used[i] != 0);
	if ((threadIdx.x & 63) == 0) {
		atomicAdd(&out2[0], (unsigned long long)__popcll(past));
		atomicAdd(&out2[1], (unsigned long long)__popcll(whole));
	}
}

// ---- the pieces --------------------------------------------------------------------------------------------------------
// pos[] holds BIT positions; in_used[] comes back in BITS from the candidate's bit; max_in and payload_end are bytes
struct BlocksPieceArgs : CarryPieceArgs {};
__global__ __launch_bounds__(64) void k_blocks_piece(BlocksPieceArgs a) { inflate_size_body<true, BlocksPieceArgs, true, true>(a); }

// one lane per candidate: a piece that stopped in front of a non-final dynamic header links to the candidate at its end bit
// (the filter passed that header if it is one); everything else to nil.  in_used[] is 0 where a piece does not decode.
__global__ __launch_bounds__(256) void k_blocks_links(const uint64_t *pos, const uint32_t *in_used, const uint32_t *stop, uint32_t ncand,
						       uint32_t *succ, uint32_t *mark)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	succ[i] = stop[i] == PIECE_NEXT ? stream_find(pos, i + 1, ncand, pos[i] + in_used[i]) : IDX_NIL;
	mark[i] = i == 0 && in_used[i];
}

// ---- the merge: the chain's pieces, in rank order, into rows ---------------------------------------------------------------
// the marked candidates' out sizes in rank order (their prefix sum is every piece's out_off); the last piece's candidate
__global__ __launch_bounds__(256) void k_blocks_sizes(const uint32_t *osize, const uint32_t *mark, const uint64_t *rank, uint32_t ncand,
						       uint64_t npieces, uint32_t *p_size, uint64_t *last)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i];
	p_size[r] = osize[i];
	if (r + 1 == npieces)
		*last = i;
}

// one lane per piece: it begins a row where it is the first, or its out_off lies in another multiple of row_bytes than
// its predecessor's (out_off ascends, so the pieces of one multiple are consecutive, and a piece is never split)
__global__ __launch_bounds__(256) void k_blocks_starts(const uint64_t *p_out, uint32_t npieces, uint64_t row_bytes, uint32_t *start)
{
	const uint32_t r = blockIdx.x * 256 + threadIdx.x;
	if (r < npieces)
		start[r] = r == 0 || p_out[r] / row_bytes != p_out[r - 1] / row_bytes;
}

// one lane per candidate: the piece that begins row k states where the row begins, in the stream (bits) and in the output.
// before[] = the exclusive prefix count of start[]; entry nrows of the two columns is the chain's end.
__global__ __launch_bounds__(256) void k_blocks_heads(const uint64_t *pos, const uint32_t *in_used, const uint32_t *osize, const uint32_t *mark,
						       const uint64_t *rank, uint32_t ncand, uint64_t npieces, const uint64_t *p_out,
						       const uint32_t *start, const uint64_t *before, uint64_t nrows, uint64_t *h_pos,
						       uint64_t *h_out)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i];
	if (start[r]) {
		h_pos[before[r]] = pos[i];
		h_out[before[r]] = p_out[r];
	}
	if (r + 1 == npieces) {
		h_pos[nrows] = pos[i] + in_used[i];
		h_out[nrows] = p_out[r] + osize[i];
	}
}

// one lane per row of the table: its four columns, the reach column cleared for k_blocks_reach.  A row of more than max_in
// bytes of stream -- a run of empty blocks, a long stretch without a dynamic header -- is named in *first (atomicMin): it
// ends the chain as a row that reaches back too far does.  (max_in < HD_INFLATE_MAX_IN, so in_len stays below 2^31 for
// every row in front of that one.)
__global__ __launch_bounds__(256) void k_blocks_rows(const uint64_t *h_pos, const uint64_t *h_out, uint32_t ntab, uint32_t max_in,
						      uint64_t *in_off, uint32_t *in_len, uint32_t *out_size, uint64_t *out_off, uint32_t *reach,
						      uint32_t *first)
{
	const uint32_t k = blockIdx.x * 256 + threadIdx.x;
	if (k >= ntab)
		return;
	const uint64_t len = h_pos[k + 1] - h_pos[k], size = h_out[k + 1] - h_out[k];
	in_off[k] = h_pos[k];
	in_len[k] = (uint32_t)len;
	out_off[k] = h_out[k];
	out_size[k] = (uint32_t)size;
	reach[k] = 0;
	if (len > 8 * (uint64_t)max_in || size > 0xffffffffull)
		atomicMin(first, k);
}

// one lane per candidate: the segmented maximum.  A piece that reaches `reach` bytes over its own first byte reaches
// reach - (its out_off - the row's out_off) over the row's, where that is above 0.
__global__ __launch_bounds__(256) void k_blocks_reach(const uint32_t *preach, const uint32_t *mark, const uint64_t *rank, uint32_t ncand,
						       const uint64_t *p_out, const uint32_t *start, const uint64_t *before, const uint64_t *h_out,
						       uint32_t ntab, uint32_t *reach)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i], k = before[r] + start[r] - 1, in = p_out[r] - h_out[k < ntab ? k : 0];
	if (k < ntab && preach[i] > in)
		atomicMax(&reach[k], (uint32_t)(preach[i] - in));
}

// w = the index's words (hd_scratch.hpp IndexWords): rows, out_bytes, end_offset, status are written, last / first / spare
// read or written as named.  The chain ends well in a piece that ended in a final block (the trailer's bytes lie behind it:
// no piece reads past the payload's end).  Otherwise it stopped in front of a header: one the filter refused -- bad where
// its bits are all there, cut where they do not fit in front of the payload's end -- or one whose piece does not decode --
// cut if its verdict is PIECE_CUT with the payload's end as its bound, bad in every other case.  Then the table's clause
// (status 3), and over it the reach rule and the long-row rule on the rows in the table (*first).  end_bit -> spare.
__global__ void k_blocks_verdict(const uint8_t *strm, const uint64_t *pos, const uint32_t *in_used, const int32_t *status, const uint32_t *stop,
				 uint32_t ncand, uint64_t npieces, uint64_t nrows, uint32_t max_rows, uint32_t max_in, uint64_t payload_end,
				 uint32_t trailer, const uint64_t *h_pos, const uint64_t *h_out, uint64_t *w)
{
	uint32_t c = 0;                                       // the piece the chain stopped in front of
	uint64_t end_bit = pos[0], end = 0, st = 0;
	if (npieces) {
		const uint32_t last = (uint32_t)w[5];
		end_bit = pos[last] + in_used[last];
		c = IDX_NIL;
		if (stop[last] != PIECE_FINAL) {
			c = stream_find(pos, last + 1, ncand, end_bit);
			if (c == IDX_NIL)
				st = block_header_at(strm, payload_end, end_bit) == BLOCK_HDR_SHORT ? 2 : 1;
		}
	}
	if (c != IDX_NIL) {
		end_bit = pos[c];
		st = status[c] == PIECE_CUT && payload_end - (end_bit >> 3) <= max_in ? 2 : 1;
	}
	uint64_t rows = nrows, upto = nrows < max_rows ? nrows : max_rows;       // status 3: the number a table must hold, the bytes of the rows it does
	if (nrows > max_rows)
		st = 3;
	const uint32_t first = (uint32_t)w[6];
	if (first != IDX_NIL) {                               // (a row of the table: k_blocks_rows, k_carry_check_reach)
		rows = upto = first;
		end_bit = h_pos[first];
		st = 1;
	}
	end = st == 0 ? ((end_bit + 7) >> 3) + trailer : end_bit >> 3;
	w[0] = rows;
	w[1] = npieces ? h_out[upto] : 0;
	w[2] = end;
	w[3] = st;
	w[7] = end_bit;
}

// ---- the decode ----------------------------------------------------------------------------------------------------------
// The check in front of the decode on a caller's table of bit rows, one lane per row: a row lies in the payload region
// [8 lo, 8 payload_end) in bits, is shorter than 2^31 bits and ends at or in front of its successor; out_off is the exclusive
// prefix sum of out_size.  *bad (0xffffffff before the launch) takes the lowest row at fault; ends[] = where the last row
// ends in the stream (bits) and in the output.  (The reach column: k_carry_check_reach.)
__global__ __launch_bounds__(256) void k_blocks_check_rows(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
							    const uint64_t *out_off, uint32_t n, uint64_t lo, uint64_t payload_end, uint32_t *bad,
							    uint64_t *ends)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t o = in_off[i], q = out_off[i], lo_bit = 8 * lo, end_bit = 8 * payload_end;
	const uint32_t len = in_len[i], size = out_size[i];
	bool fault = len >= 0x80000000u || o < lo_bit || o > end_bit || len > end_bit - o || (i == 0 && q != 0);
	if (i + 1 < n) {
		fault = fault || in_off[i + 1] < o || in_off[i + 1] - o < len || out_off[i + 1] - q != size || out_off[i + 1] < q;
	} else {
		ends[0] = o + len;
		ends[1] = q + size;
	}
	if (fault)
		atomicMin(bad, i);
}

// k_carry_decode for a row that starts at bit in_off & 7 of byte in_off >> 3 and is in_len BITS long: it ends behind a final
// block, or behind a block that ends on bit in_len exactly; a block end past in_len fails the row, as more than out_size
// symbols or a distance over reach do
struct BlocksDecodeArgs : CarryDecodeArgs {};
#define HD_ROWS_DECODE_KERNEL k_blocks_decode
#define HD_ROWS_DECODE_ARGS BlocksDecodeArgs
#define HD_ROWS_DECODE_BITS true
#include "hd_rows_decode.hpp"

} // namespace hd
