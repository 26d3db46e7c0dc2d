// hd_stream.hpp -- ONE gzip / zlib / raw DEFLATE stream from a device buffer, coded in parallel chunks.
//
// Role: the single-stream writers of the reference -- zlibstdio / zlibrawstdio (zlibrawstdio_compress.h:260-307), the IDAT
// of applet/7png.c:296-331 -- which are one serial deflate() there.  Here the buffer is cut into chunks, every chunk is an
// ordinary block of the batch encoder in HD_FRAME_RAW_FLUSH form (such chunks concatenate), the chunks are gathered behind
// a header, and the CRC-32 / Adler-32 of the whole input is FOLDED from the chunks' checksums:
//   k_stream_table    chunk i's in_off / in_len;
//   k_chunk_adler     the Adler-32 of every chunk (the encode kernels return the CRC-32 themselves);
//   k_check_combine   the fold, one lane per part, no serial chain: part i contributes check[i] moved over the S_i bytes
//                     behind it, and the contributions add (XOR for the CRC, sums mod 65521 for Adler);
//   k_stream_ends     header, 03 00 and trailer.
// The inverse (k_stream_check_table, k_stream_trailer) holds a stream and its chunk table to the same rules, so that the
// chunks can be inflated side by side: the device-resident form of what a dictzip reader does with its RA table.
#pragma once
#include "hd_compact.hpp"
#include "hd_index.hpp"
#include "hd_inflate_size.hpp"

namespace hd {

constexpr uint32_t CHECK_CRC32 = 0, CHECK_ADLER32 = 1;   // `kind` of the fold
constexpr uint32_t ADLER_MOD = 65521u;
constexpr uint32_t FOLD_GRID = 256;                      // workgroups of k_check_combine at most: 65536 parts per trip

// ---- GF(2)[x] / P in reflected bit order (x^0 is bit 31): hd_host_util.h's gf_xpow for the device, on hd_device.hpp's
// gf_mul.  x^(2^k), k = 0..63, is a table the compiler works out.
constexpr uint32_t gf_mul_const(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (uint32_t m = 1u << 31; m; m >>= 1) {
		p ^= (a & m) ? b : 0u;
		b = (b >> 1) ^ ((b & 1) ? 0xedb88320u : 0u);
	}
	return p;
}

struct GfPow2 {
	uint32_t v[64];
};
constexpr GfPow2 gf_pow2_table()
{
	GfPow2 t{};
	uint32_t sq = 1u << 30;
	for (int k = 0; k < 64; k++) {
		t.v[k] = sq;
		sq = gf_mul_const(sq, sq);
	}
	return t;
}
constexpr GfPow2 GF_POW2_VALUES = gf_pow2_table();
static __constant__ const GfPow2 GF_POW2 = GF_POW2_VALUES;

// x^(8 n) for any n < 2^64: x^n from the table, then three squarings -- 8 n is never formed
__device__ __forceinline__ uint32_t gf_xpow8(uint64_t n)
{
	uint32_t p = 1u << 31;
	for (uint32_t k = 0; n; n >>= 1, k++)
		if (n & 1)
			p = gf_mul(p, GF_POW2.v[k]);
	p = gf_mul(p, p);
	p = gf_mul(p, p);
	return gf_mul(p, p);
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t s)
{
	for (int o = 32; o > 0; o >>= 1)
		s += ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)s, o, 64)) |
		     ((uint64_t)(uint32_t)__shfl_down((int)(uint32_t)(s >> 32), o, 64) << 32);
	return s;
}

// The fold.  prefix[] is the exclusive 64-bit scan of len[], *total its sum: S_i = total - prefix[i] - len[i] bytes lie
// behind part i.  A part of length 0 is an identity whatever its check says.
//   CRC-32    acc[0] ^= check[i] * x^(8 S_i)
//   Adler-32  acc[0] += a_i - 1,  acc[1] += b_i + (a_i - 1) (S_i mod 65521), every term reduced mod 65521 first: a lane adds
//             at most 2^16 terms below 2^16, the accumulators at most 2^32 of them
// acc[] is zero before the launch; wavefronts reduce in registers, workgroups through LDS, the grid with one vector atomic
// per workgroup and accumulator.  k_check_combine_finish makes the check of it.
__global__ __launch_bounds__(256) void k_check_combine(const uint32_t *__restrict__ check, const uint32_t *__restrict__ len,
							const uint64_t *__restrict__ prefix, const uint64_t *__restrict__ total,
							uint32_t n, uint32_t kind, uint64_t *acc)
{
	__shared__ uint64_t wa[4], wb[4];
	const uint32_t t = threadIdx.x;
	const uint64_t T = *total;
	uint64_t a = 0, b = 0;
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + t; i < n; i += (uint64_t)gridDim.x * 256) {
		const uint32_t L = len[i];
		if (!L)
			continue;
		const uint64_t S = T - prefix[i] - L;
		const uint32_t c = check[i];
		if (kind == CHECK_CRC32) {
			a ^= gf_mul(c, gf_xpow8(S));
		} else {
			const uint32_t a1 = ((c & 0xffffu) + ADLER_MOD - 1u) % ADLER_MOD;
			a += a1;
			b += ((c >> 16) % ADLER_MOD + (uint64_t)a1 * (uint32_t)(S % ADLER_MOD)) % ADLER_MOD;
		}
	}
	if (kind == CHECK_CRC32) {
		uint32_t x = (uint32_t)a;
		for (int o = 32; o > 0; o >>= 1)
			x ^= (uint32_t)__shfl_down((int)x, o, 64);
		a = x;
	} else {
		a = wave_sum64(a);
		b = wave_sum64(b);
	}
	if ((t & 63) == 0) {
		wa[t >> 6] = a;
		wb[t >> 6] = b;
	}
	__syncthreads();
	if (t == 0) {
		if (kind == CHECK_CRC32) {
			const uint32_t x = (uint32_t)(wa[0] ^ wa[1] ^ wa[2] ^ wa[3]);
			if (x)
				atomicXor((uint32_t *)acc, x);
		} else {
			atomicAdd((unsigned long long *)acc, (unsigned long long)(wa[0] + wa[1] + wa[2] + wa[3]));
			atomicAdd((unsigned long long *)acc + 1, (unsigned long long)(wb[0] + wb[1] + wb[2] + wb[3]));
		}
	}
}

// ... and *carry, the check of everything in front of these parts (0 / 1 where there is nothing), becomes the check of
// both: the carry is one more part with *total bytes behind it.  total == NULL: no parts, the carry stays.
__global__ void k_check_combine_finish(const uint64_t *acc, const uint64_t *total, uint32_t kind, uint32_t *carry)
{
	if (threadIdx.x)
		return;
	const uint64_t T = total ? *total : 0;
	const uint32_t c = *carry;
	if (kind == CHECK_CRC32) {
		*carry = gf_mul(c, gf_xpow8(T)) ^ (uint32_t)acc[0];
	} else {
		const uint32_t ca = ((c & 0xffffu) + ADLER_MOD - 1u) % ADLER_MOD;
		const uint32_t A = (uint32_t)((1u + ca + acc[0] % ADLER_MOD) % ADLER_MOD);
		const uint32_t B = (uint32_t)(((c >> 16) % ADLER_MOD + ((uint64_t)ca * (uint32_t)(T % ADLER_MOD)) % ADLER_MOD +
					       acc[1] % ADLER_MOD) % ADLER_MOD);
		*carry = (B << 16) | A;
	}
}

// one lane per chunk of a window: chunk first + i of the input
__global__ __launch_bounds__(256) void k_stream_table(uint32_t first, uint32_t n, uint32_t chunk_bytes, uint64_t nbytes,
						       uint64_t *in_off, uint32_t *in_len)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t o = ((uint64_t)first + i) * chunk_bytes, left = nbytes - o;
	in_off[i] = o;
	in_len[i] = left < chunk_bytes ? (uint32_t)left : chunk_bytes;
}

// The Adler-32 of base[off[i] .. + len[i]) for every i, one wavefront each, in the loop of k_adler32_patch; where `cap` is
// given no more than cap[i] bytes are read (the decode side: what an inflate that failed left in out_len does not matter).
__global__ __launch_bounds__(64) void k_chunk_adler(const uint8_t *__restrict__ base, const uint64_t *__restrict__ off,
						     const uint32_t *__restrict__ len, const uint32_t *__restrict__ cap, uint32_t n,
						     uint32_t *__restrict__ adler)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= n)
		return;
	const uint8_t *src = base + off[b];
	uint32_t nb = len[b];
	if (cap && cap[b] < nb)
		nb = cap[b];
	const bool aligned = (((uintptr_t)src) & 15) == 0;
	AdlerLanes adl;
	adl.init();
	for (uint32_t piece = 0; (uint64_t)piece * HD_PIECE < nb; piece++) {
		const uint32_t o = piece * HD_PIECE + lane * 16;
		uint4 v = make_uint4(0, 0, 0, 0);
		if (aligned && (uint64_t)o + 16 <= nb) {
			v = *(const uint4 *)(src + o);
		} else if (o < nb) {
			uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
			for (uint32_t k = 0; k < 16; k++)
				w[k >> 2] |= (o + k < nb ? (uint32_t)src[o + k] : 0u) << (8 * (k & 3));
			v = make_uint4(w[0], w[1], w[2], w[3]);
		}
		adl.fold(piece, lane, v);
	}
	const uint32_t a = adl.finish(nb);
	if (lane == 0)
		adler[b] = a;
}

__device__ __forceinline__ uint32_t stream_header_bytes(int frame) { return frame == HD_FRAME_GZIP ? 10u : frame == HD_FRAME_ZLIB ? 2u : 0u; }
__device__ __forceinline__ uint32_t stream_trailer_bytes(int frame) { return frame == HD_FRAME_GZIP ? 8u : frame == HD_FRAME_ZLIB ? 4u : 0u; }

// The two ends of the stream, one wavefront, a byte per lane: lanes 0..15 the header at dst (78 da | 1f 8b 08 00 <mtime 0>
// 02 00), lanes 16..31 the empty final block 03 00 and the trailer at dst + end (Adler-32 big-endian | CRC-32, ISIZE
// little-endian); end -> chunk_off_end where the caller keeps a table.
__global__ __launch_bounds__(64) void k_stream_ends(uint8_t *dst, int frame, uint64_t end, const uint32_t *check, uint32_t isize,
						     uint64_t *chunk_off_end)
{
	const uint32_t lane = threadIdx.x;
	const uint32_t c = *check;
	if (lane < 16) {
		const uint64_t h = frame == HD_FRAME_GZIP ? 0x00088b1full : 0xda78ull;
		if (lane < stream_header_bytes(frame))
			dst[lane] = lane < 8 ? (uint8_t)(h >> (8 * lane)) : lane == 8 ? (uint8_t)2 : (uint8_t)0;
	} else if (lane < 32) {
		const uint32_t k = lane - 16;
		uint8_t v = k == 0 ? (uint8_t)3 : (uint8_t)0;
		if (k >= 2) {
			const uint32_t j = k - 2;
			if (frame == HD_FRAME_ZLIB)
				v = (uint8_t)(c >> (24 - 8 * (j & 3)));
			else
				v = (uint8_t)((j < 4 ? c : isize) >> (8 * (j & 3)));
		}
		if (k < 2 + stream_trailer_bytes(frame))
			dst[end + k] = v;
	} else if (lane == 32 && chunk_off_end) {
		*chunk_off_end = end;
	}
}

// ---- decode ---------------------------------------------------------------------------------------------------------
// One lane per entry of chunk_off[0 .. nchunks]: entry i < nchunks is chunk i -- it must start at or behind the header,
// in front of its successor, and end (with every chunk behind it) in front of the terminator's place, nbytes - 2 -
// trailer, shorter than HD_INFLATE_MAX_IN; entry nchunks is the 03 00, which must lie exactly there, and it answers for
// the header's bytes too.  *bad (0xffffffff before the launch) takes the lowest entry at fault.  The rows of the inflate's
// tables are written in any case (length 0 where the entry is at fault); the inflate runs only where nothing is.
// No byte of strm at or behind nbytes is read: the host has made sure that nbytes >= header + 2 + trailer.
__global__ __launch_bounds__(256) void k_stream_check_table(const uint8_t *strm, uint64_t nbytes, const uint64_t *chunk_off,
							     uint32_t nchunks, uint32_t chunk_bytes, uint64_t out_bytes, int frame,
							     uint64_t *in_off, uint32_t *in_len, uint64_t *out_off, uint32_t *out_cap,
							     uint32_t *bad)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i > nchunks)
		return;
	const uint64_t hdr = stream_header_bytes(frame), limit = nbytes - 2 - stream_trailer_bytes(frame);
	const uint64_t o = chunk_off[i];
	bool fault;
	if (i < nchunks) {
		const uint64_t nx = chunk_off[i + 1];
		fault = o < hdr || o >= nx || nx > limit || nx - o >= HD_INFLATE_MAX_IN;
		const uint64_t at = (uint64_t)i * chunk_bytes, left = out_bytes - at;
		in_off[i] = o;
		in_len[i] = fault ? 0u : (uint32_t)(nx - o);
		out_off[i] = at;
		out_cap[i] = left < chunk_bytes ? (uint32_t)left : chunk_bytes;
	} else {
		fault = o < hdr || o != limit;
		if (!fault)
			fault = strm[o] != 3 || strm[o + 1] != 0;
		if (frame == HD_FRAME_GZIP) {
			fault = fault || strm[0] != 0x1f || strm[1] != 0x8b || strm[2] != 8 || strm[3] != 0;        // FLG 0: ten bytes
		} else if (frame == HD_FRAME_ZLIB) {
			const uint32_t cmf = strm[0], flg = strm[1];
			fault = fault || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20) || ((cmf << 8) | flg) % 31 != 0;
		}
	}
	if (fault)
		atomicMin(bad, i);
}

// the folded check (and the length) against the trailer
__global__ void k_stream_trailer(const uint8_t *strm, uint64_t nbytes, int frame, uint64_t out_bytes, const uint32_t *check,
				 uint32_t *mismatch)
{
	if (threadIdx.x)
		return;
	const uint32_t c = *check;
	uint32_t bad = 0;
	if (frame == HD_FRAME_ZLIB) {
		const uint8_t *t = strm + nbytes - 4;
		bad = (((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3]) != c;
	} else if (frame == HD_FRAME_GZIP) {
		const uint8_t *t = strm + nbytes - 8;
		const uint32_t crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
		const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
		bad = crc != c || isize != (uint32_t)out_bytes;
	}
	*mismatch = bad;
}

// ---- the index of a stream nobody kept a table for -----------------------------------------------------------------------
// A chunk in flush form ends in an empty stored block, and that block's last four bytes are 00 00 ff ff on a byte boundary.
// This is hd_index.hpp's problem again, with a decoder in the place of the header rules:
//   1. k_stream_flag / k_stream_write: one streaming read of the payload region finds every position with those four bytes
//      in front of it; with the first payload byte they are the sorted candidate list;
//   2. k_inflate_piece (hd_inflate_size.hpp), one wavefront per candidate, decodes from there to the first flush point or
//      final block; its distance check makes a chunk that reaches back over its own start bad data from that start;
//   3. k_stream_links: a piece that ends in a flush point links to the candidate at its end;
//   4. k_index_jump marks what candidate 0 reaches, a prefix count ranks it, k_stream_rows writes the tables;
//   5. k_stream_verdict names where the chain stopped and why.

// bit k: the four bytes at o + k are 00 00 ff ff and o + k >= lo; the candidate is the byte behind them.  The passes get
// the payload's end less one as their nbytes, so a marker that ends on the last payload byte, or runs into the trailer,
// makes no candidate.
struct MatchFlush {
	static constexpr uint32_t SHIFT = 4;
	uint64_t lo;
	__device__ __forceinline__ uint32_t operator()(const uint32_t (&d)[5], uint64_t o) const
	{
		uint32_t m = 0;
#pragma unroll
		for (uint32_t k = 0; k < 16; k++) {
			const uint32_t w = (k & 3) ? __builtin_amdgcn_alignbyte(d[(k >> 2) + 1], d[k >> 2], k & 3) : d[k >> 2];
			m |= (uint32_t)(w == 0xffff0000u) << k;
		}
		if (o < lo)
			m = lo - o >= 16 ? 0u : m & ~((1u << (uint32_t)(lo - o)) - 1u);
		return m;
	}
};

__global__ __launch_bounds__(256) void k_stream_flag(const uint8_t *strm, uint64_t nbytes, uint64_t lo, uint64_t *bitmap, uint32_t *tile_cnt)
{
	index_flag_body(strm, nbytes, bitmap, tile_cnt, MatchFlush{ lo });
}

__global__ __launch_bounds__(256) void k_stream_write(const uint8_t *strm, uint64_t nbytes, uint64_t lo, const uint64_t *bitmap,
						       uint64_t nwords, const uint64_t *tile_off, uint64_t *pos)
{
	index_write_body(strm, nbytes, bitmap, nwords, tile_off, pos, MatchFlush{ lo });
}

// the candidate at offset `at` among pos[from .. ncand), IDX_NIL if there is none
__device__ __forceinline__ uint32_t stream_find(const uint64_t *pos, uint32_t from, uint32_t ncand, uint64_t at)
{
	uint32_t lo = from, hi = ncand;
	while (lo < hi) {
		const uint32_t mid = lo + ((hi - lo) >> 1);
		if (pos[mid] < at)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < ncand && pos[lo] == at ? lo : IDX_NIL;
}

// one lane per candidate: a piece that ended in a flush point links to the candidate behind it (there is one unless the
// payload ends there), everything else to nil.  in_used[] is 0 where a piece does not decode.
__global__ __launch_bounds__(256) void k_stream_links(const uint64_t *pos, const uint32_t *in_used, const uint32_t *stop, uint32_t ncand,
						       uint32_t *succ, uint32_t *mark)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand)
		return;
	succ[i] = stop[i] == PIECE_FLUSH ? stream_find(pos, i + 1, ncand, pos[i] + in_used[i]) : IDX_NIL;
	mark[i] = i == 0 && in_used[i];                      // the head of the true chain
}

// the marked candidates in rank order -> the rows; the last one is named in *last
__global__ __launch_bounds__(256) void k_stream_rows(const uint64_t *pos, const uint32_t *in_used, const uint32_t *osize,
						      const uint32_t *mark, const uint64_t *rank, uint32_t ncand, uint64_t nrows,
						      uint32_t max_chunks, uint64_t *in_off, uint32_t *in_len, uint32_t *out_size, uint64_t *last)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= ncand || !mark[i])
		return;
	const uint64_t r = rank[i];
	if (r < max_chunks) {
		in_off[r] = pos[i];
		in_len[r] = in_used[i];
		out_size[r] = osize[i];
	}
	if (r + 1 == nrows)
		*last = i;
}

// sum[] = { nchunks, out_bytes, end_offset, status, -, the last row's candidate }.  The chain ends well in a piece that
// ended in a final block (the trailer's bytes lie behind it: no piece reads past the payload's end); it is cut where a
// flush point is the payload's last byte; otherwise it stopped in front of a piece that does not decode, and that piece is
// cut if its verdict is PIECE_CUT with the payload's end as its bound, bad in every other case.
__global__ void k_stream_verdict(const uint64_t *pos, const uint32_t *in_used, const int32_t *status, const uint32_t *stop,
				 uint32_t ncand, uint64_t nrows, uint32_t max_chunks, uint32_t max_in, uint64_t payload_end, uint32_t trailer,
				 uint64_t *sum)
{
	uint32_t c = 0;                                       // the piece the chain stopped in front of
	uint64_t end = 0, st = 0;
	if (nrows) {
		const uint32_t last = (uint32_t)sum[5];
		end = pos[last] + in_used[last];
		if (stop[last] == PIECE_FINAL) {
			end += trailer;
			c = IDX_NIL;
		} else {
			c = stream_find(pos, last + 1, ncand, end);
			if (c == IDX_NIL)
				st = 2;
		}
	}
	if (c != IDX_NIL) {
		end = pos[c];
		st = status[c] == PIECE_CUT && payload_end - end <= max_in ? 2 : 1;
	}
	if (nrows > max_chunks)
		st = 3;
	sum[0] = nrows;
	sum[2] = end;
	sum[3] = st;
}

// The check in front of the decode on a caller's table of uneven rows, one lane per row: a row lies in the payload region
// [lo, payload_end), is shorter than HD_INFLATE_MAX_IN and ends at or in front of its successor; out_off is the exclusive
// prefix sum of out_size.  *bad (0xffffffff before the launch) takes the lowest row at fault; ends[] = where the last row
// ends in the stream and in the output.
__global__ __launch_bounds__(256) void k_stream_check_rows(const uint64_t *in_off, const uint32_t *in_len, const uint32_t *out_size,
							    const uint64_t *out_off, uint32_t n, uint64_t lo, uint64_t payload_end,
							    uint32_t *bad, uint64_t *ends)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n)
		return;
	const uint64_t o = in_off[i], q = out_off[i];
	const uint32_t len = in_len[i], size = out_size[i];
	bool fault = len >= HD_INFLATE_MAX_IN || o < lo || o > payload_end || len > payload_end - o || (i == 0 && q != 0);
	if (i + 1 < n) {
		fault = fault || in_off[i + 1] < o || in_off[i + 1] - o < len || out_off[i + 1] - q != size || out_off[i + 1] < q;
	} else {
		ends[0] = o + len;
		ends[1] = q + size;
	}
	if (fault)
		atomicMin(bad, i);
}

} // namespace hd
