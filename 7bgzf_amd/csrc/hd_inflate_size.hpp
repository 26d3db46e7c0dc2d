// hd_inflate_size.hpp -- the size pass: how many bytes a DEFLATE stream decodes to, without decoding them.
//
// Role: the first of the two inflates of applet/7png.c:114-181, which runs the IDAT stream into a throw-away buffer only
// to count declen, and the "get decompressed size" call of other device DEFLATE libraries: a stream whose size nobody
// stated.  One wavefront per stream, the throughput decoder (hd_inflate.hpp) with everything taken out that moves bytes:
//
//   kept   everything that READS the stream, and it is the shared code of hd_inflate_common.hpp, used directly: the bit
//          reader (InfReader), the block headers (inflate_dynamic_header / inflate_static_tables over build_table), the
//          window decode (spec_token per lane, window_walk along the chain); the checked token of the scalar path is a
//          copy of the full decoder's, its litlen lookup from LDS -- so EVERY verdict of the full decoder: table rejects,
//          over-subscribed codes, input overrun, a distance past the bytes out so far; LEN / NLEN is checked here;
//   gone   the ring, the window's output budget, the flush, the copies, the CRC, the tables' copy in registers.
//
// What is left of the output is its position: 64 bits, and a stream that reaches 2^32 bytes is answered
// HD_INSUFFICIENT_SPACE where it does -- what the full decoder answers in the largest room its 32-bit tables can state.
// The distance check `offset > pos` can fail only while fewer than 32 KiB are out and is skipped afterwards, as the
// front of k_inflate_lat does.  A stored block is a seek.
//
// LDS: the two direct tables, the sorted symbols and counts of the slow path, and one union of the code lengths (header)
// with the stream copy (windows): 4288 bytes = four 1280-byte allocation units, 32 wavefronts per CU (k_inflate: five, 25);
// at most 64 VGPRs keep the registers from being the tighter bound (tests/test_abi.py holds both).
#pragma once
#include "hd_inflate.hpp"

namespace hd {

struct SizeArgs {
	const uint8_t *in;
	const uint64_t *p_off;           // the DEFLATE payloads: the caller's own tables (HD_FRAME_RAW) or k_frame_open's
	const uint32_t *p_len;
	const uint64_t *m_off;           // where each member starts (its header counts into in_used); nullptr: at p_off
	const int32_t *verdict;          // k_frame_open's verdict on the header; nullptr: no headers
	uint32_t nblocks;
	uint32_t trailer;                // bytes behind the stream: 0, 4 (Adler-32: not examined) or 8 (CRC-32: not examined, ISIZE: examined)
	uint32_t *out_size;
	uint32_t *in_used;
	int32_t *status;
};

struct InfSizeLds {
	uint32_t lit[1u << INF_LT_BITS];
	uint32_t off[1u << INF_DT_BITS];
	uint16_t lit_sorted[288];
	uint16_t off_sorted[32];
	uint16_t lit_count[16], off_count[16];
	union {
		struct {
			uint8_t cl[288 + 32 + 138 + 6];   // + worst-case RLE overrun; the table builder's scratch at INF_T_SCRATCH
			uint8_t pre_lens[32];
		};
		uint32_t comp[128];                   // 2 pieces of the compressed stream for the window decoder
	};
};
static_assert(sizeof(InfSizeLds) <= 4 * 1280, "InfSizeLds must stay within four LDS allocation units");

// The piece form (k_inflate_piece): the same decoder started at a candidate of the stream index (hd_stream.hpp), which
// stops at whichever comes first -- a flush point, the end of a non-final stored block with LEN == 0, or the end of a
// final block -- and says which.  Its input is the candidate's bytes up to the end of the payload region, max_in at
// the most.  Every verdict of the size pass is kept, and one is told apart: PIECE_CUT where the decoder needed a bit at
// or behind the end of its input (bits there read as 0; whatever the decoder makes of them, the verdict is this one).
struct PieceArgs {
	const uint8_t *in;
	const uint64_t *pos;             // the candidates, ascending
	uint32_t ncand;
	uint32_t max_in;                 // < HD_INFLATE_MAX_IN
	uint64_t payload_end;            // > pos[i] for every i
	uint32_t *out_size;
	uint32_t *in_used;               // whole bytes, 0 where the piece does not decode
	int32_t *status;                 // HD_OK | HD_BAD_DATA | HD_INSUFFICIENT_SPACE | PIECE_CUT
	uint32_t *stop;                  // PIECE_FLUSH | PIECE_FINAL, 0 where the piece does not decode
};
constexpr int32_t PIECE_CUT = 4;
// The member form (k_inflate_member, hd_index.hpp): a piece that is the DEFLATE stream of a gzip member nobody stated the
// length of.  Candidate sub[b] of pos[] starts a member whose header k_member_open measured (hdr[], and status[] HD_OK; any
// other status: nothing is decoded and every column stays); its window ends at nbytes or max_in bytes behind the
// candidate, whichever comes first.  The only stop is the end of a final block -- a flush point is none -- and behind it
// the trailer's eight bytes must lie inside the window (PIECE_CUT where they do not) and its ISIZE equal the decoded
// length (HD_BAD_DATA).  osize[] = that length, total[] = header + stream + 8; both 0 where status[] is not HD_OK.
struct MemberArgs {
	const uint8_t *in;
	const uint64_t *pos;             // every candidate of the index
	const uint32_t *sub;             // the ncand of them to size; the five columns below are indexed by candidate
	uint32_t ncand;
	uint32_t max_in;                 // < HD_INFLATE_MAX_IN
	uint64_t nbytes;                 // > pos[i] for every i
	const uint32_t *hdr;
	uint32_t *osize;
	uint32_t *total;
	int32_t *status;                 // HD_OK | HD_BAD_DATA | HD_INSUFFICIENT_SPACE | PIECE_CUT
};
constexpr uint32_t PIECE_FLUSH = 1, PIECE_FINAL = 2, PIECE_NEXT = 3, PIECE_PAST_HEADER = 4;
// The carried form (k_carry_piece, hd_carry.hpp): a piece of a stream whose writer kept the window across the flush.  A
// distance past the bytes the piece has put out is no fault then -- 32768 is DEFLATE's most, and the bytes in front of the
// piece are another row's -- and reach[] takes the furthest one: 0 where the piece stands alone.
struct CarryPieceArgs : PieceArgs {
	uint32_t *reach;
};
// The block form (k_blocks_piece, hd_blocks.hpp): a carried piece of a stream without flush points.  pos[] holds BIT
// positions and the piece starts on its bit; it stops behind a final block, or behind a non-final block with BFINAL 0 /
// BTYPE 2 in the three bits behind it (PIECE_NEXT: the next non-final dynamic header) -- a flush point is no stop -- and
// in_used[] is in BITS from the candidate's bit.  A piece that does not decode but got past its own first block header -- the
// tables of a dynamic block built, LEN / NLEN of a stored one agreeing -- says so in stop[] (PIECE_PAST_HEADER: a count for
// the bench, no link and no verdict looks at it).

template <bool PIECE, class Args, bool CARRY = false, bool BITS = false, bool MEMBER = false> __device__ __forceinline__ void inflate_size_body(const Args &a)
{
	__shared__ InfSizeLds L;
	const uint32_t lane = threadIdx.x;
	const uint32_t b = blockIdx.x;
	uint64_t p_off;
	uint32_t n;
	[[maybe_unused]] uint32_t sh = 0;              // (block form) the candidate's bit in its byte
	[[maybe_unused]] uint32_t row = b;             // (member form) the candidate this wavefront sizes
	if constexpr (MEMBER) {
		if (b >= a.ncand)
			return;
		row = a.sub[b];
		if (a.status[row] != HD_OK)                // the header did not fit the window
			return;
		const uint64_t p = a.pos[row], left = a.nbytes - p;
		const uint32_t h = a.hdr[row];             // < the window: k_member_open
		p_off = p + h;
		n = (left < a.max_in ? (uint32_t)left : a.max_in) - h;
	} else if constexpr (PIECE) {
		if (b >= a.ncand)
			return;
		p_off = a.pos[b];
		if constexpr (BITS) {
			sh = (uint32_t)p_off & 7;
			p_off >>= 3;
		}
		const uint64_t left = a.payload_end - p_off;
		n = left < a.max_in ? (uint32_t)left : a.max_in;
	} else {
		if (b >= a.nblocks)
			return;
		p_off = a.p_off[b];
		n = a.p_len[b];
	}
	const uint8_t *src = a.in + p_off;
	if constexpr (!PIECE) {
		if (n >= HD_INFLATE_MAX_IN || (a.verdict && a.verdict[b])) {
			// (stream positions are 32-bit bit counts, as in k_inflate: a stream this long is refused whole)
			if (lane == 0) {
				a.out_size[b] = 0;
				a.in_used[b] = 0;
				a.status[b] = HD_BAD_DATA;
			}
			return;
		}
	}

	InfReader R(src, n, lane);
	if constexpr (BITS)
		R.drop(sh);
	uint64_t pos = 0;                              // bytes the stream has decoded to so far (uniform)
	[[maybe_unused]] uint32_t reach = 0;           // (carried form) the furthest a match went back over the piece's first byte
	constexpr uint64_t POS_LIMIT = 0xffffffffull;  // the largest room a u32 table states: past it the answer is "does not fit"

	// ---- window decode: the throughput decoder's, without its byte work --------------------------------------------------
	// Every lane decodes the tokens that would start at bit B + lane and B + 64 + lane; the scalar walk (the same
	// statement) follows the real chain and stops in front of the first token a window cannot take.  There is no budget
	// to cut at: what the real tokens put out is one prefix sum, and its total moves the position.
	// Returns 0 = one token through the scalar path, 2 = error (st set).
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
			// (the fields that place bytes -- the entry, the literals' mask -- are not looked at: the compiler drops them)
			const InfSpec s0 = spec_token(L, bl0, ws0, ws1, ws2), s1 = spec_token(L, bl0 + 64, ws2, ws3, ws4);
			uint32_t wb, wm;
			uint64_t real0, real1;
			window_walk(s0.walk, s1.walk, wb, real0, real1, wm);
			if (real0 == 0)
				break;                                     // the token at B is not for a window: scalar path
			// (both halves' output lengths in one prefix sum, 16 bits each: 64 x 258 < 2^16)
			const uint32_t scn = wave_incl_scan(sel(real0, s0.outlen, 0u) | (sel(real1, s1.outlen, 0u) << 16));
			const uint32_t tot = readlane(scn, 63);
			if (pos < 32768) {
				// offset > bytes out so far (decompress_template.h:724): only this early can it be
				const uint32_t opos0 = (uint32_t)pos + (scn & 0xffff) - s0.outlen;
				const uint32_t opos1 = (uint32_t)pos + (scn >> 16) + (tot & 0xffff) - s1.outlen;
				const uint64_t far0 = __ballot(opos0 < s0.offset), far1 = __ballot(opos1 < s1.offset);
				if ((far0 & real0 & s0.is_len) | (far1 & real1 & s1.is_len)) {
					if constexpr (CARRY) {
						uint32_t r = max(sel(far0 & real0 & s0.is_len, s0.offset - opos0, 0u),
								 sel(far1 & real1 & s1.is_len, s1.offset - opos1, 0u));
						for (int o = 32; o > 0; o >>= 1)
							r = max(r, (uint32_t)__shfl_xor((int)r, o, 64));
						reach = max(reach, uniform(r));
					} else {
						st_out = HD_BAD_DATA;
						result = 2;
						break;
					}
				}
			}
			pos += (tot & 0xffff) + (tot >> 16);
			B += wb;
			if (pos > POS_LIMIT) {
				st_out = HD_INSUFFICIENT_SPACE;
				result = 2;
				break;
			}
			if (wm & 64)
				break;                                     // the walk stopped in front of a long codeword or the end of the block
		}
		R.seek_bit(B);
		return result;
	};

	int32_t st = HD_OK;
	bool static_loaded = false;
	uint32_t stop = 0;                            // (piece form) the stop it hit
	[[maybe_unused]] bool past = false;           // (block form) the first block's header is behind the decoder
	bool cut = false;                             // (piece form) a stored block's LEN / NLEN or payload reaches past the input
	for (;;) {
		R.refill();
		lds_p0 = 0xfffffff0u;                     // header parsing reuses the LDS behind L.comp
		const uint32_t bfinal = (uint32_t)R.bb & 1;
		const uint32_t btype = ((uint32_t)R.bb >> 1) & 3;
		R.drop(3);

		if (btype == 0) {
			// ---- stored (decompress_template.h:234-279): a seek ------------
			const int64_t cbits = (R.consumed_bits() + 7) & ~(int64_t)7;
			if (cbits > 8 * (int64_t)n) { st = HD_BAD_DATA; break; }
			uint32_t ip = (uint32_t)(cbits >> 3);
			if (n - ip < 4) { st = HD_BAD_DATA; cut = true; break; }
			R.seek_byte(ip);
			R.refill();
			const uint32_t len = (uint32_t)R.bb & 0xffff, nlen = ((uint32_t)R.bb >> 16) & 0xffff;
			ip += 4;
			if (len != (~nlen & 0xffff)) { st = HD_BAD_DATA; break; }
			if constexpr (BITS)
				past = true;
			if (pos + len > POS_LIMIT) { st = HD_INSUFFICIENT_SPACE; break; }
			if (len > n - ip) { st = HD_BAD_DATA; cut = true; break; }
			pos += len;
			R.seek_byte(ip + len);
			if constexpr (PIECE && !BITS && !MEMBER) {
				if (!bfinal && len == 0) {
					stop = PIECE_FLUSH;
					break;
				}
			}
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

			if constexpr (BITS)
				past = true;
			// ---- symbol loop ----------------------------------------------
			for (;;) {
				if (uniform(run_windows(st)))
					break;
				// one token through the fully checked scalar path (stream edges, long codes, end of block); the
				// tables are read from LDS: no copy of them in registers, this kernel answers to occupancy.  (pos <= POS_LIMIT
				// here).  Own copy of the token decode, as in inflate_stream and inflate_stream_pipe: a shared function lost 0.3-0.9 % here
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
					if (pos == POS_LIMIT) { st = HD_INSUFFICIENT_SPACE; break; }
					pos++;
					continue;
				}
				if (kind == K_EOB)
					break;
				const uint32_t eb = (e >> 4) & 15;
				const uint32_t length = (e >> 16) + ((uint32_t)R.bb & ((1u << eb) - 1));
				R.drop(eb);
				if (length > POS_LIMIT - pos) { st = HD_INSUFFICIENT_SPACE; break; }
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
				if (offset > pos) {                                  // decompress_template.h:724
					if constexpr (CARRY) {
						reach = max(reach, offset - (uint32_t)pos);
					} else {
						st = HD_BAD_DATA;
						break;
					}
				}
				pos += length;
			}
			if (st != HD_OK)
				break;
		}
		if (bfinal) {
			if constexpr (PIECE)
				stop = PIECE_FINAL;
			break;
		}
		if (R.consumed_bits() > 8 * (int64_t)n + 64) { st = HD_BAD_DATA; break; }
		if constexpr (BITS) {
			R.refill();
			if (((uint32_t)R.bb & 7) == 4) {             // BFINAL 0, BTYPE 2: with bit 2 set, all three are the stream's own
				stop = PIECE_NEXT;
				break;
			}
		}
	}
	if constexpr (MEMBER) {
		// cut as a piece is; then the trailer behind the byte the stream ended on (used <= n)
		if (cut || R.consumed_bits() > 8 * (int64_t)n)
			st = PIECE_CUT;
		uint32_t used = 0;
		if (st == HD_OK) {
			used = (uint32_t)((R.consumed_bits() + 7) >> 3);
			if (n - used < 8) {
				st = PIECE_CUT;
			} else {
				const uint8_t *t = src + used + 4;
				const uint32_t isize = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
				if (isize != (uint32_t)pos)
					st = HD_BAD_DATA;
			}
		}
		if (lane == 0) {
			a.osize[row] = st == HD_OK ? (uint32_t)pos : 0u;
			a.total[row] = st == HD_OK ? (uint32_t)(p_off - a.pos[row]) + used + 8u : 0u;
			a.status[row] = st;
		}
	} else if constexpr (PIECE) {
		// with the decoder's position past the input -- at a stop it reached through the zero bits, or at the failure they
		// led to -- the piece is cut, whatever else the decoder found there
		if (cut || R.consumed_bits() > 8 * (int64_t)n)
			st = PIECE_CUT;
		if (lane == 0) {
			a.out_size[b] = st == HD_OK ? (uint32_t)pos : 0u;
			if constexpr (BITS)
				a.in_used[b] = st == HD_OK ? (uint32_t)(R.consumed_bits() - sh) : 0u;
			else
				a.in_used[b] = st == HD_OK ? (uint32_t)((R.consumed_bits() + 7) >> 3) : 0u;
			a.status[b] = st;
			a.stop[b] = st == HD_OK ? stop : BITS && past ? PIECE_PAST_HEADER : 0u;
			if constexpr (CARRY)
				a.reach[b] = st == HD_OK ? reach : 0u;
		}
	} else {
		if (st == HD_OK && R.consumed_bits() > 8 * (int64_t)n)
			st = HD_BAD_DATA;

		// ---- the verdict: the stream's, and the one field of the trailer that needs no byte of output ----
		uint32_t used = 0;
		if (st == HD_OK) {
			used = (uint32_t)((R.consumed_bits() + 7) >> 3);
			if (a.trailer == 8) {
				// RFC 1952 ISIZE, behind the CRC-32 (gzip_decompress.c:124-127); used <= n, and k_frame_open left 8 bytes behind n
				const uint8_t *t = src + used + 4;
				const uint32_t isize = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
				if (isize != (uint32_t)pos)
					st = HD_BAD_DATA;
			}
		}
		if (lane == 0) {
			const uint32_t hdr = a.m_off ? (uint32_t)(p_off - a.m_off[b]) : 0u;
			a.out_size[b] = st == HD_OK ? (uint32_t)pos : 0u;
			a.in_used[b] = st == HD_OK ? hdr + used + a.trailer : 0u;
			a.status[b] = st;
		}
	}
}

__global__ __launch_bounds__(64) void k_inflate_size(SizeArgs a) { inflate_size_body<false>(a); }
__global__ __launch_bounds__(64) void k_inflate_piece(PieceArgs a) { inflate_size_body<true>(a); }
__global__ __launch_bounds__(64) void k_inflate_member(MemberArgs a) { inflate_size_body<true, MemberArgs, false, false, true>(a); }

} // namespace hd
