// hd_deflate_static.hpp -- level 1: greedy LZ77 + static Huffman, one wavefront
// per block, streaming bit emission (BASELINE config 2).
//
// Replaces, for BGZF_METHOD=hip1, what libdeflate_deflate (lib/zlibutil.c:179)
// -> deflate_compress_fastest (lib/libdeflate/deflate_compress.c:2453-2524)
// -> deflate_flush_block (:1707-2038) do per block on one CPU thread, and the
// CRC-32 of the block (fcrc32, applet/7bgzf.c:269) and the BGZF/MiGz framing
// (applet/7bgzf.c:263-272, applet/7migz.c:224-233) that the applet adds.
//
// The parse is wave64-native (oracle/hd_deflate_twin.c is its serial twin and
// must produce the same bytes):
//   lanes stand on 64 consecutive positions S..S+63; each hashes its 4 bytes,
//   reads the candidate from the 16-bit LDS hash table, then publishes itself
//   (conflicts inside a step are re-written until the largest position holds the
//   slot); candidates are verified against the LDS ring window, 8 bytes per lane;
//   the greedy choice of token starts is a DPP prefix scan over 8-state
//   transition functions (two v_perm_b32 per composition; every lane's function is
//   elementary -- the lanes the last step's match covers are literals -- so the
//   scan's first three stages shift one dword, not two); the rare matches whose
//   8 bytes all agree are extended cooperatively, 64 bytes per ballot; the step's
//   tokens are compacted into a queue -- a register, filled by a cross-lane push
//   whose result joins it one step later, so that no step waits for it --
//   and once 64 wait there one pass turns them into static-Huffman codes, places
//   them with a DPP prefix scan of their bit lengths and ORs them into a small LDS
//   staging ring, whose whole dwords leave in front of the next pass.
//
// HBM traffic per block: input read once (16 B/lane pieces), output written
// once.  LDS per wave at level 1: ring 2^WIN_BITS + 16 + table (2 B x HD_TABLE_ENTRIES)
// + 256 B staging = 7440 B: 6 of the 1280-byte units LDS is granted in, 21 waves
// per CU (with the 1 KiB staging ring and the 640 B LDS queue it had been 8848 B, 7
// units, 18 waves).  The level-2 parse (TOK) keeps its LDS queue and its 7 units.
#pragma once
#include <type_traits>
#include "hd_device.hpp"

namespace hd {

constexpr uint32_t HD_HINT_NO_WHOLE = 1;   // no block is short enough to be coded whole
constexpr uint32_t HD_HINT_NO_SEG = 2;     // no block is long enough to be coded in segments
constexpr uint32_t BESIDE_KEEP_MAX = 3;    // emit wavefronts a CU keeps at most beside a parse workgroup (k_deflate_dynamic<..., BESIDE>)

struct DeflateArgs {
	const uint8_t *in;
	const uint64_t *in_off;
	const uint32_t *in_len;
	uint32_t nblocks;
	int frame;
	int level;
	uint8_t *out;
	uint64_t out_stride;
	uint32_t out_cap;
	uint32_t *out_len;
	uint32_t *crc;
	int32_t *status;
	const CrcTables *ct;
	uint8_t *scratch;               // token slabs of the dynamic levels
	uint32_t first;                 // split path: first block of this sub-batch (grid index 0)
	uint32_t count;                 // split path: blocks in this sub-batch
	uint32_t skip_small;            // fused dynamic kernel: leave blocks <= split_max to the split path
	uint32_t split_max;             // split path: largest block it takes (sizes the scratch layout)
	uint32_t *split_ovf;            // split path: per block, 1 = left to the fused kernel (too many tokens)
	uint32_t seg_limit;             // level-1 and fused dynamic kernel: != 0 = leave longer blocks alone (hd_segment.hpp codes them)
	uint32_t seg_bytes;             // ... as segments of this size (HD_SEG_BYTES, or HD_LAT_SEG_BYTES in latency mode)
	// host side only (latency contexts, which see the lengths): launches known to have nothing to do are left out,
	// and the segment table comes ready-made in device-visible memory instead of from k_seg_table
	uint32_t hint;                  // HD_HINT_*
	const uint64_t *host_seg_off;
	const uint32_t *host_seg_len;
	// split path, latency segments of the dynamic levels (HD_LAT_PARTS): != 0 = every block of in_off/in_len is PARSED
	// as this many parts of HD_LAT_PART_BYTES, one wavefront each, and emitted as one DEFLATE block by one
	uint32_t parts = 0;
	// != 0: in_off / in_len are the segment table of a latency-mode launch with this many slots per block; a segment that
	// is not the first of its block is PRIMED with the HD_LAT_PRIME_BYTES before it (the end of its predecessor)
	uint32_t seg_slots = 0;
	// latency contexts: the last launch of a run (k_seg_finish) tells the host it is done by itself -- its last workgroup
	// stores `done_epoch` into `done_flag` (pinned host memory) behind a system-scope fence -- so the caller polls a word
	// instead of going through hipStreamSynchronize.  done_count: a device word the workgroups count themselves off on
	uint32_t *done_flag = nullptr, *done_count = nullptr;
	uint32_t done_epoch = 0;
	// != 0: the records in `scratch` are the workgroup parse's (hd_deflate_wg.hpp wg_layout: a token per byte, a DEFLATE
	// block per HD_WG_SPLIT_MIN bytes); the emit-only kernel reads them so
	uint32_t wg = 0;
	// the workgroup levels, HD_FRAME_LATENCY: a handful of blocks, each wanted back soon -- the member is written by a
	// WORKGROUP (hd_emit_wg.hpp k_emit_wg: the same bytes as the one-wavefront emit kernel, sixteen wavefronts at them)
	uint32_t lat = 0;
	// ... and the PARSE of one block is shared by this many workgroups (k_parse_wg, a.lat launches of a few blocks: 1, 2 or 4):
	// workgroup q replays the table stores of the pieces in front of its range -- hashes and bucket updates only, in the same
	// order, so its table is what the one workgroup's would be there -- and parses its own range; same tokens, a fraction of
	// the time a lone block spends on one CU.  0 = 1
	uint32_t wg_split = 0;
	// ... reading it from here (device memory: block i of the sub-batch at stage_in + i * 64 KiB, put there by k_stage_in)
	// instead of a.in -- which for a latency context is the caller's pinned memory: four readers of a block over PCIe
	// cost more than the shared parse gains
	const uint8_t *stage_in = nullptr;
	// a device word that counts the blocks the workgroup parse gave up on because a turn did not come (WG_SPIN_LIMIT;
	// they are written stored): hipdeflate_stall_count()
	uint32_t *stalls = nullptr;
	// the workgroup levels' throughput form, emit BESIDE the parse (hd_deflate_wg.hpp launch_wg): ready[32 * i] != 0 once block
	// first + i's records are complete (raised by its parse workgroup; the emit wavefront that has the block waits for it; a
	// flag per 128-byte line), arrived counts the emit wavefronts that are resident (the parse is launched behind a gate on it)
	uint32_t *ready = nullptr, *arrived = nullptr, *next = nullptr;     // (next: the counter the blocks are handed out by)
	// ... SPAN: the emit kernel serves the WHOLE launch -- sub-batch k = blocks [k * span_sub, ...) has its records in `scratch` (k even)
	// or `scratch_b` (k odd), its flag at ready[32 * b] for the launch's block b, and emitted[k] counts its members as they are done
	// (the parse of sub-batch k + 2, which overwrites the records, is launched behind a gate on it)
	uint32_t span_sub = 0;
	uint8_t *scratch_b = nullptr;
	uint32_t *emitted = nullptr;
	// ... and in front of that gate a launch of the emit kernel that takes what is left of sub-batch k and of no other (take_sub = k + 1;
	// SPAN hands the blocks out by a counter per sub-batch, next[k]): whatever became of the resident wavefronts, every block of
	// sub-batch k has a live taker before the gate waits.  Should the gate give up all the same (~8 s: a device in trouble), it sets
	// *poison and the parses behind it leave the records alone -- their blocks are written stored and counted as stalls, valid
	// streams, not the twin's bytes
	uint32_t take_sub = 0;
	uint32_t *poison = nullptr;
	uint32_t beside_keep = BESIDE_KEEP_MAX;      // emit wavefronts a CU keeps (tests: hipdeflate_test_beside(keep = 0): nobody stays)
	// the workgroup levels' throughput form: the most history a block may use, 0 or HD_WG_WINDOW.  != 0: block b is parsed with the
	// min(prime_max, in_off[b]) & ~(HD_WG_CUT - 1) bytes in front of it in the table and the window (k_primed_wg: no token for them, its
	// CRC-32 the block's alone, distances up to 32768 into them) -- a.in + in_off[b] is then one buffer's offset, not any address
	uint32_t prime_max = 0;
	// host side only: a WgBeside (hd_deflate_wg.hpp) -- the second stream and the events of that scheme; nullptr = emit behind parse
	void *beside = nullptr;
};

__host__ __device__ __forceinline__ uint32_t frame_hdr_bytes(int frame)
{
	return frame == HD_FRAME_BGZF ? 18u : frame == HD_FRAME_MIGZ ? 20u : frame == HD_FRAME_ZLIB ? 2u
	     : frame == HD_FRAME_GZIP ? 10u : 0u;
}

// CRC32 + ISIZE behind the gzip-family members, Adler-32 behind RFC 1950
__host__ __device__ __forceinline__ uint32_t frame_trl_bytes(int frame)
{
	return frame == HD_FRAME_ZLIB ? 4u : (frame == HD_FRAME_BGZF || frame == HD_FRAME_MIGZ || frame == HD_FRAME_GZIP) ? 8u : 0u;
}

// 16-bit field `k` of the trailer: CRC32 then ISIZE; the four Adler-32 bytes of an
// RFC 1950 member are left zero here, k_adler32_patch writes them
__device__ __forceinline__ uint32_t frame_trl_field(int frame, uint32_t k, uint32_t crc, uint32_t n)
{
	const uint32_t w = k < 2 ? (frame == HD_FRAME_ZLIB ? 0u : crc) : n;
	return (w >> (16 * (k & 1))) & 0xffff;
}

// HD_FRAME_RAW_FLUSH: room kept for the flush suffix (3 header bits + alignment, 00 00 ff ff)
__device__ __forceinline__ uint32_t frame_sfx_bytes(int frame)
{
	return frame == HD_FRAME_RAW_FLUSH ? 5u : 0u;
}

// segment slots per block (hd_segment.hpp): enough for the longest block whose worst case fits the slot
__host__ __device__ inline uint32_t seg_slots_per_block(uint32_t cap, uint32_t seg)
{
	const uint32_t full = HD_STORED_SIZE(seg) + 5u;
	// (a raw frame has no header, a flush frame no 03 00 tail -- its shortest last segment, one byte, takes
	// 1 + 5 + 5 = 11 bytes: the count may be one high for the other frames, never low)
	return cap / full + (cap % full >= 11u ? 1u : 0u);
}

// THE rule for which blocks of a launch are coded in segments (hd_segment.hpp) and which the ordinary coding takes -- the
// segment table, the stitch and the finish, the level-1 kernel, level 2's parse, emit and fused kernel and the latency
// contexts' host table all ask this one question.  (Here rather than in hd_segment.hpp: the ordinary kernels come first.)
//   limit == 0 (every launch of blocks no longer than it; the headline): none.
//   the throughput form (seg = HD_SEG_BYTES), and any block longer than HD_SEG_LIMIT: every block longer than `limit`,
//     refused by the stitch when the room is below HD_SEG_WORST -- as the twin's twin_segmented().
//   latency segments: a block longer than `limit` whose room covers the latency form's worst case; a longer block in a
//     smaller room gets the ordinary form, as the twin and the per-block codecs give it (the twin's twin()).
__host__ __device__ inline bool seg_coded(uint32_t len, uint32_t limit, uint32_t seg, int frame, uint64_t out_stride, uint32_t out_cap)
{
	if (!limit || len <= limit)
		return false;
	if (seg == HD_SEG_BYTES || len > HD_SEG_LIMIT)
		return true;
	uint64_t room = out_stride < out_cap ? out_stride : out_cap;
	const uint32_t S = seg_slots_per_block(room > 0x7fffffffu ? 0x7fffffffu : (uint32_t)room, seg);
	if (frame == HD_FRAME_BGZF && room > 65536)
		room = 65536;
	return HD_SEGN_COUNT(len, seg) <= S &&
	       frame_hdr_bytes(frame) + HD_SEGN_WORST((uint64_t)len, seg, frame == HD_FRAME_RAW_FLUSH) + frame_trl_bytes(frame) <= room;
}

// Levels 1..2 in a launch that codes nothing in segments (its room is at most HD_SEG_LIMIT -- HD_LAT_SEG_BYTES in latency
// mode): a block longer than HD_SEG_LIMIT has no form but the segmented one, whose worst case exceeds the block and so the
// room -- refused, as the twin refuses it, instead of coded whole
__device__ __forceinline__ bool whole_refused(const DeflateArgs &a, uint32_t n)
{
	return a.level >= 1 && !a.seg_limit && n > HD_SEG_LIMIT;
}

__device__ __forceinline__ void refuse_member(const DeflateArgs &a, uint32_t b, uint32_t lane)
{
	if (lane == 0) {
		a.out_len[b] = 0;
		if (a.status) a.status[b] = 1;
		if (a.crc) a.crc[b] = 0;
	}
}

// dword `j` (0..3) of the container header with its size field zero
__device__ __forceinline__ uint32_t frame_hdr_word(int frame, uint32_t j)
{
	// BGZF / MiGz: 1f 8b 08 04 | 00 00 00 00 | 00 ff XL 00 | S1 S2 SL 00     applet/7bgzf.c:263-265
	// gzip:        1f 8b 08 00 | mtime = 0   | 02 00                          lib/zlibutil.c:380-386
	// zlib:        78 da                                                       lib/zlibutil.c:375-376
	const bool bz = frame == HD_FRAME_BGZF, gz = frame == HD_FRAME_GZIP, zl = frame == HD_FRAME_ZLIB;
	const uint32_t w0 = zl ? 0x0000da78u : gz ? 0x00088b1fu : 0x04088b1fu;
	const uint32_t w2 = zl ? 0u : gz ? 0x00000002u : bz ? 0x0006ff00u : 0x0008ff00u;
	const uint32_t w3 = (zl || gz) ? 0u : bz ? 0x00024342u : 0x00045a4du;
	return j == 0 ? w0 : j == 1 ? 0u : j == 2 ? w2 : w3;
}

// byte `o` of the container header; `sizefield` = BSIZE (u16) or compsize (u32)
__device__ __forceinline__ uint32_t frame_hdr_byte(int frame, uint32_t o, uint32_t sizefield)
{
	const uint32_t w = o < 16 ? frame_hdr_word(frame, o >> 2) : sizefield;
	return (w >> (8 * (o & 3))) & 0xff;
}

// Stored-block form of the whole member, written from scratch (fallback when
// the Huffman stream would not be smaller, deflate_compress.c:1820-1856; the
// guarantee that a 0xff00-byte BGZF block always fits).
__device__ __forceinline__ void write_stored_member(const DeflateArgs &a, uint32_t b, const uint8_t *src, uint32_t n,
						  uint32_t crc, uint32_t lane)
{
	const uint32_t hdr = frame_hdr_bytes(a.frame), trl = frame_trl_bytes(a.frame);
	const bool flush = a.frame == HD_FRAME_RAW_FLUSH;   // no final block; empty stored block 00 | 00 00 ff ff behind
	const uint32_t stored = HD_STORED_SIZE(n);
	const uint32_t total = hdr + stored + trl + (flush ? 5u : 0u);
	uint64_t cap = a.out_stride < a.out_cap ? a.out_stride : a.out_cap;
	if (a.frame == HD_FRAME_BGZF && cap > 65536)
		cap = 65536;
	if (total > cap) {
		if (lane == 0) {
			a.out_len[b] = 0;
			if (a.status) a.status[b] = 1;
			if (a.crc) a.crc[b] = crc;
		}
		return;
	}
	const uint32_t sizefield = a.frame == HD_FRAME_BGZF ? total - 1 : stored;
	const uint32_t nblk = n == 0 ? 1u : (n + 65534u) / 65535u;
	uint32_t *dst32 = (uint32_t *)(a.out + (uint64_t)b * a.out_stride);
	for (uint32_t j = lane; j < (total + 3) / 4; j += 64) {
		uint32_t w = 0;
		for (uint32_t k = 0; k < 4; k++) {
			uint32_t o = 4 * j + k, v = 0;
			if (o < hdr) {
				v = frame_hdr_byte(a.frame, o, sizefield);
			} else if (o < hdr + stored) {
				uint32_t q = (o - hdr) / 65540u, r = (o - hdr) - q * 65540u;
				uint32_t left = n - q * 65535u;
				uint32_t bl = left < 65535u ? left : 65535u;
				if (r == 0) v = (q + 1 == nblk && !flush) ? 1u : 0u;
				else if (r == 1) v = bl & 0xff;
				else if (r == 2) v = bl >> 8;
				else if (r == 3) v = ~bl & 0xff;
				else if (r == 4) v = (~bl >> 8) & 0xff;
				else v = src[q * 65535u + r - 5];
			} else if (o < total) {
				uint32_t t = o - hdr - stored;
				v = flush ? (t >= 3 ? 0xffu : 0u) : (frame_trl_field(a.frame, t >> 1, crc, n) >> (8 * (t & 1))) & 0xff;
			}
			w |= v << (8 * k);
		}
		dst32[j] = w;
	}
	if (lane == 0) {
		a.out_len[b] = total;
		if (a.status) a.status[b] = 0;
		if (a.crc) a.crc[b] = crc;
	}
}

// load the 16 bytes of slot (piece, lane); zero beyond n
__device__ __forceinline__ uint4 load_slot(const uint8_t *src, uint32_t n, uint32_t piece, uint32_t lane, bool aligned)
{
	const uint32_t o = piece * HD_PIECE + lane * 16;
	if (aligned && o + 16 <= n)
		return *(const uint4 *)(src + o);
	// ragged tail or unaligned source: byte loads, zero beyond n (static indices
	// only -- a runtime-indexed array would live in scratch)
	uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
	if (o < n) {
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			w0 |= (o + k < n ? (uint32_t)src[o + k] : 0u) << (8 * k);
			w1 |= (o + 4 + k < n ? (uint32_t)src[o + 4 + k] : 0u) << (8 * k);
			w2 |= (o + 8 + k < n ? (uint32_t)src[o + 8 + k] : 0u) << (8 * k);
			w3 |= (o + 12 + k < n ? (uint32_t)src[o + 12 + k] : 0u) << (8 * k);
		}
	}
	return make_uint4(w0, w1, w2, w3);
}

// ---- dynamic levels: parse kernel -> HBM -> emit kernel ------------------------
// Per block of a sub-batch the scratch holds the member's tokens (at most one per
// input byte), the symbol histograms of its DEFLATE blocks (a block closes at the
// first step boundary with >= HD_DYN_BLOCK_TOKENS tokens) and a small record.  The
// parse is this file's kernel with TOK = true: the same steps, but the token queue
// drains into the slab and the histograms instead of into static-Huffman bits.
// hd_deflate_dynamic.hpp's kernel in its emit-only mode turns that into the bytes
// the fused kernel would have written.  The layout is sized by the largest block
// the launch admits (a.split_max: the slot stride bounds it) and holds one token
// per TWO input bytes: compressible data stays well below that (DNA-like 0.2,
// text 0.35 tokens per byte); a block that does not (noise) sets its flag in
// a.split_ovf and is taken by the fused kernel afterwards, as are blocks larger
// than split_max, if any.
//   [ tokens: cap_tok x u32 | ndb, crc, pad, pad | ntok[max_db] | hist[max_db][320] ]
struct SplitLayout {
	uint32_t cap_tok, max_db;
	uint64_t off_rec, off_ntok, off_hist, bytes;
};
// full: room for one token per byte -- the parts of a latency segment (HD_LAT_PARTS), which have no fused kernel behind them
__host__ __device__ inline SplitLayout split_layout(uint32_t max_block, bool full = false)
{
	SplitLayout l;
	// three tokens per four input bytes: text parsed with the short-table levels comes close to one per two
	// (level 4 on the enwik-like set overflowed half its blocks at max_block / 2: 51 GB/s instead of 95)
	l.cap_tok = full ? ((max_block + 64 + 15) & ~15u) : max_block / 4 * 3 + 128;
	l.max_db = l.cap_tok / HD_DYN_BLOCK_TOKENS + 2;
	l.off_rec = (uint64_t)l.cap_tok * 4;
	l.off_ntok = l.off_rec + 16;
	l.off_hist = (l.off_ntok + (uint64_t)l.max_db * 4 + 15) & ~(uint64_t)15;
	l.bytes = l.off_hist + (uint64_t)l.max_db * 320 * 4;
	return l;
}
__device__ __forceinline__ uint8_t *split_block(uint8_t *scratch, uint32_t max_block, uint32_t i)
{
	return scratch + (uint64_t)i * split_layout(max_block).bytes;
}
// the record of part `i` (counted over the sub-batch: segment * parts + part) of a latency segment
__host__ __device__ inline SplitLayout part_layout() { return split_layout(HD_LAT_PART_BYTES, true); }
__device__ __forceinline__ uint8_t *part_block(uint8_t *scratch, uint32_t i)
{
	return scratch + (uint64_t)i * part_layout().bytes;
}

// TOK: the parse kernel of level 2 (hd_deflate_dynamic.hpp), in level 2's geometry; INTRA: its in-step candidates (HD_INTRA_DIST)
// PRIMED: the instantiation latency-mode launches use -- parts and priming (HD_LAT_PRIME) are compiled in.  The parse kernel
// always has them; the level-1 kernel of the 16 GiB runs does not (with them in, 0.5 % slower for nothing)
template <int WIN_BITS, int HASH_BITS, bool TOK, int INTRA = 0, bool PRIMED = TOK>
__global__ __launch_bounds__(64) void k_deflate_static(DeflateArgs a)
{
	static_assert(PRIMED || !TOK, "the parse kernels are always built with the latency-mode paths");
	static_assert(!TOK || (WIN_BITS == HD_L2_WIN_BITS && HASH_BITS == HD_L2_HASH_BITS && HD_L2_MIN_LEN == HD_MIN_MATCH),
		      "the parse kernel is level 2's: its ring, its table, its minimum length");
	constexpr uint32_t W = 1u << WIN_BITS;
	constexpr uint32_t W4M = W / 4 - 1;
	constexpr uint32_t HS = HD_TABLE_ENTRIES(WIN_BITS, HASH_BITS);
	// staging ring, dwords: one emit pass adds at most 64 x 31 bits = 62 dwords, and every whole dword leaves in front
	// of a pass, so at most one partial dword is live then: 1 + 62 + 1 (the spill-over slot put() always ORs into)
	constexpr uint32_t STG = 64;
	constexpr uint32_t TOKQ = 128;           // TOK: token queue in LDS, < 64 waiting + <= 64 of one step
	// K16: every lane whose first eight bytes agree learns bytes 8..15 in the vector domain too (four more ring
	// dwords per lane), so the scalar extension loop below runs only for matches of 16 bytes and more.  On text
	// 98 % of the "long" matches are 9..15 bytes long, and the parse kernel waits on that loop's LDS round trip;
	// the level-1 kernel is bound by its vector instruction count instead and keeps the loop
	constexpr bool K16 = TOK;

	// + 16 bytes that mirror the start of the ring, so that the 3 dwords under an
	// unaligned 8-byte read never wrap
	__shared__ __attribute__((aligned(W))) uint32_t ring32[W / 4 + 4];       // W-aligned: ring address = (x & (W - 1)) | base
	// (position + 1) mod 2^16, 0 = empty
	__shared__ __attribute__((aligned(16))) uint16_t table[HS];
	// TOK: no bits are made here, the staging ring's place is taken by the symbol histograms
	// (316 counters: litlen [0,286), offset [286,316), 32 bits wide: packed 16-bit ones measured 4 % slower
	// where they bought no wave)
	__shared__ __attribute__((aligned(16))) uint32_t stage[TOK ? 316 : STG];
	// TOK: tokens waiting for the emit pass.  Level 1 keeps them in a register (Q0 below) and has no such array:
	// ring 4112 + table 3072 + staging 256 = 7440 B, six 1280-byte units where the LDS queue made it seven
	__shared__ uint32_t tokbuf[TOKQ];
	const uint32_t ring_lds = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)ring32;   // LDS byte address of the ring

	const uint32_t lane = threadIdx.x;
	// PARTS (TOK, a.parts != 0): wavefront = part blockIdx.x % parts of segment a.first + blockIdx.x / parts.  A part behind
	// the first one starts HD_LAT_PRIME_BYTES early: those steps fill table and window and their tokens are dropped
	const bool parted = PRIMED && TOK && a.parts != 0;
	const uint32_t b = a.first + (parted ? blockIdx.x / a.parts : blockIdx.x);
	if (b >= a.nblocks)
		return;
	const ClockStamp clk(TOK ? HD_CLK_PARSE : HD_CLK_STATIC);
	const uint8_t *src = a.in + a.in_off[b];
	uint32_t n = a.in_len[b];
	// PRIMED (latency mode): the wavefront starts `prime` bytes ahead of what it codes and runs those steps as the front of
	// the pipeline only -- table and window are warm when its own bytes begin, and its first matches may reach back
	uint32_t prime = (PRIMED && HD_LAT_SEG_PRIME && a.seg_slots && b % a.seg_slots) ? HD_LAT_PRIME(HD_LAT_PRIME_BYTES, n) : 0u;
	if (parted) {
		const uint32_t o = (blockIdx.x % a.parts) * HD_LAT_PART_BYTES;
		if (o >= n)
			return;                              // the segment ends before this part (the emit wave knows)
		n = n - o < HD_LAT_PART_BYTES ? n - o : HD_LAT_PART_BYTES;
		prime = o ? HD_LAT_PRIME(o, n) : HD_LAT_PRIME(prime, n);
		src += o;
	}
	const uint8_t *const src_own = src;          // what this wavefront codes: [src_own, src_own + n_own)
	const uint32_t n_own = n;
	src -= prime;
	n += prime;
	// (a block coded in segments is flagged too: the emit kernel passes it over, and so does the fused kernel)
	if (TOK && !parted && (n > a.split_max || seg_coded(n_own, a.seg_limit, a.seg_bytes, a.frame, a.out_stride, a.out_cap))) {
		if (lane == 0)
			a.split_ovf[b] = 1;
		return;                              // the fused kernel takes the large blocks
	}
	if (!TOK && seg_coded(n_own, a.seg_limit, a.seg_bytes, a.frame, a.out_stride, a.out_cap))
		return;                              // coded in segments (hd_segment.hpp)
	if (!TOK && whole_refused(a, n_own)) {
		refuse_member(a, b, lane);
		return;
	}
	const bool aligned = (((uintptr_t)src) & 15) == 0;
	uint32_t *dst32 = (uint32_t *)(a.out + (uint64_t)b * a.out_stride);
	const CrcTables *ct = a.ct;

	const uint32_t hdr = frame_hdr_bytes(a.frame), trl = frame_trl_bytes(a.frame);
	uint64_t cap64 = a.out_stride < a.out_cap ? a.out_stride : a.out_cap;
	if (a.frame == HD_FRAME_BGZF && cap64 > 65536)
		cap64 = 65536;
	const uint32_t cap = (uint32_t)cap64;
	const uint32_t stored = HD_STORED_SIZE(n_own);
	// the static stream survives only while it stays strictly below the stored
	// size and inside the slot (twin: deflate_static(), `limit`)
	uint32_t limit = stored - 1;
	const bool flush = a.frame == HD_FRAME_RAW_FLUSH;
	const uint32_t sfx = frame_sfx_bytes(a.frame);
	bool use_static = TOK || (a.level >= 1 && cap >= hdr + trl + sfx + 2);   // level 0: stored only
	if (!TOK && use_static && cap - hdr - trl - sfx < limit)
		limit = cap - hdr - trl - sfx;
	const uint32_t limit_bits = limit > 0x1fffffe0u ? 0xffffff00u : 8u * limit;    // (the per-step test in 32 bits; a stream of 2^32 bits is out of the kernel's reach anyway)

	// ---- init LDS -------------------------------------------------------
	for (uint32_t i = lane; i < HS / 8; i += 64)
		((uint4 *)table)[i] = make_uint4(0, 0, 0, 0);
	for (uint32_t i = lane; i < (TOK ? 316u : STG); i += 64)
		stage[i] = 0;
	if (!TOK && lane < 4 && hdr)
		stage[lane] = frame_hdr_word(a.frame, lane);
	// TOK: where this block's tokens, histograms and record go
	const SplitLayout lay = parted ? part_layout() : split_layout(TOK ? a.split_max : 0);
	uint8_t *const rec = !TOK ? nullptr : parted ? part_block(a.scratch, blockIdx.x) : split_block(a.scratch, a.split_max, blockIdx.x);
	uint32_t *const slab = (uint32_t *)rec;
	uint32_t ntok_slab = 0, db_start = 0, ndb = 0;       // tokens stored; first token / index of the open DEFLATE block
	int32_t db_room = HD_DYN_BLOCK_TOKENS;               // tokens until the open DEFLATE block may close (stored + queued ones counted)

	Fn8Ident fid;
	fid.init(lane);
	Fn8Cross fcross;                     // the cross-row stages' identity registers: read by fn8_scan_state0 alone
	fcross.init(lane);
	// level 1, the steps of a group: the lane number with the match token's constant part on it, K = HD_TOKEN_MATCH_TAG -
	// (3 << 16).  pk = S + lane_k is the step's position register there: pk - c is the token word's base whole, and the one
	// other reader of the position, the long-match events, masks its addresses into the ring (K's low 16 bits are zero).
	// Opaque, as Fn8Cross is: the compiler cannot make it again from `lane`, an add per step
	uint32_t lane_k = lane + (HD_TOKEN_MATCH_TAG - (3u << 16));
	asm volatile("" : "+v"(lane_k));
	HashConsts hk;
	hk.init(HS);
	CrcLanes crc;
	// (a primed part's CRC covers [prime, n): the lanes of the priming bytes -- all in the first piece -- fold zeros from
	// state 0, which leaves them at 0, and the register's all-ones start sits on the part's first slot)
	crc.init(lane, n, prime);
	uint32_t filled = 0;                 // ring holds [max(0,filled-W), filled)
	uint4 pre = load_slot(src, n, 0, lane, aligned);

	uint32_t bitpos = 8 * hdr;           // absolute bit position in the slot
	uint32_t flushed = 0;                // dwords already stored to HBM
	const uint32_t paybase = 8 * hdr;

	// OR one token per lane (nbits == 0: none) into the staging ring
	auto put = [&](uint32_t code, uint32_t nbits, uint32_t incl, uint32_t total) {
		// branch-free: a lane without a token ORs zeros; the second dword gets the
		// bits that spill over (zero when the token does not cross a dword)
		const uint32_t bp = bitpos + incl - nbits;
		const uint32_t sh = bp & 31, i = (bp >> 5) & (STG - 1);
		const uint64_t wide = (uint64_t)code << sh;                    // callers pass code = 0 where nbits = 0
		atomicOr(&stage[i], (uint32_t)wide);
		atomicOr(&stage[(i + 1) & (STG - 1)], (uint32_t)(wide >> 32));
		bitpos += total;
	};
	// every whole dword staged so far leaves (at most 63: what one put() left), one contiguous 4-byte-per-lane store, and its
	// place in the ring is zero again.  Called in front of every emit pass and of the member's tail, so that the ring only
	// ever has to hold one partial dword and what comes then (a pass: 62 dwords; the tail: four)
	// In two halves, for the emit pass, which waits for its table gather between them: the LDS half reads the lane's dword
	// and zeroes its place (in front of the pass's put(), which ORs into it again), the store half sends it to HBM.
	// (Two divergent regions on purpose.  In one, with the wait inside, the compiler waits again where the lanes join --
	// vmcnt(0), the store included.  `fl` is pinned so that both halves share it; `v` starts undefined, not zero: the
	// lanes that do not drain never store it, and a zero would be a v_mov per pass)
	auto drain_read = [&](uint32_t &fl) -> uint32_t {
		const uint32_t ready = (bitpos >> 5) - flushed;
		fl = flushed + lane;
		asm("" : "+v"(fl));
		uint32_t v;
		asm("" : "=v"(v));
		if (lane < ready) {
			const uint32_t i = fl & (STG - 1);
			v = stage[i];
			stage[i] = 0;
		}
		return v;
	};
	auto drain_store = [&](uint32_t fl, uint32_t v) {
		const uint32_t ready = (bitpos >> 5) - flushed;
		if (lane < ready)
			dst32[fl] = v;
		flushed = bitpos >> 5;
	};
	auto drain = [&]() {
		uint32_t fl;
		const uint32_t v = drain_read(fl);
		drain_store(fl, v);
	};
	// vmcnt counts vector-memory operations in issue order: a wait for a younger one cannot pass before every older one
	// is back.  The next piece is an HBM miss (the input is streamed once) that nothing needs for 16 steps, so it is
	// requested BEHIND the CRC's twenty table gathers and their waits -- the youngest operation, which nothing waits for.
	// (Requested first, as it was, the gathers' first wait -- vmcnt(18) of 21 outstanding -- stood for the whole HBM round
	// trip at the head of every 16-step group.)  The fence keeps the compiler from moving the load back up.
	auto crc_then_prefetch = [&](uint32_t piece, uint4 v) {
		crc.fold(ct, piece, piece * HD_PIECE + lane * 16 + 16 <= n && piece * HD_PIECE + lane * 16 >= prime, v);
		asm volatile("" : "+v"(crc.s) : : "memory");
		if (filled < n)
			pre = load_slot(src, n, piece + 1, lane, aligned);
	};
	auto fill_piece = [&]() {
		const uint32_t piece = filled / HD_PIECE;
		const uint4 v = pre;
		filled += HD_PIECE;
		const uint32_t ro = (piece * HD_PIECE) & (W - 1);
		((uint4 *)ring32)[ro / 16 + lane] = v;
		if (ro == 0 && lane == 0)
			((uint4 *)ring32)[W / 16] = v;          // mirror of ring bytes [0,16)
		crc_then_prefetch(piece, v);
	};
	// ---- the front of the pipeline -------------------------------------------
	// A step is split in three stages that run one iteration apart, so that no
	// LDS round trip is waited for where it is issued:
	//   fetch(k+2)  own 8 bytes at S + lane, hash, table lookup, publish
	//   probe(k+1)  the three ring dwords under the candidate found by fetch
	//   compute(k)  verify, scan, codes, emit
	// The table holds (position + 1) mod 2^16 in 16 bits (0 = empty): half the
	// LDS of 32-bit entries, which buys occupancy.  Several lanes of a step may
	// publish to one slot in the same store instruction: the highest lane (the
	// largest position) stays, which is the result the CPU twin computes.
	struct Fetched {
		uint32_t v, vh, c;           // own bytes [p,p+4), [p+4,p+8); candidate position + 1 (0 = none)
	};
	// INNER: every lane of the step has >= 9 bytes left and the block is shorter than
	// 2^16 (all BGZF blocks; all but their last steps), so the end-of-block and the
	// 16-bit wrap-around handling drop out at compile time
	// OWN_AHEAD (the parse kernels, which run two to four waves per SIMD and wait where level 1 issues): the three ring
	// dwords under a lane's own position are read ONE STEP AHEAD of the fetch that hashes them -- a fourth pipeline
	// stage -- so that the table lookup no longer waits for an LDS round trip inside its own step
	// MEASURED AND SWITCHED OFF (round 3, same box): level 6 116.9 -> 112.2 GB/s, level 5 148.8 -> 143.4, level 9 68.2 -> 64.7:
	// at two waves per SIMD every instruction costs its issue slot, the hand-over copies and seven more registers cost
	// more than the round trip they hide.  (And not for the level-2 geometry in any case: 99 VGPRs would cost it a wave.)
	constexpr bool OWN_AHEAD = false;
	struct Own {
		uint32_t w0, w1, w2;
	};
	auto own = [&](uint32_t S_) -> Own {
		const uint32_t *w = &ring32[((S_ + lane) >> 2) & W4M];
		Own o = { w[0], w[1], w[2] };
		return o;
	};
	Own o1 = { 0, 0, 0 };                     // OWN_AHEAD: the dwords under S + 192 + lane
	auto fetch = [&](auto inner_tag, uint32_t S_) -> Fetched {
		constexpr bool INNER = decltype(inner_tag)::value;
		Fetched f;
		const uint32_t p = S_ + lane;
		const uint32_t *w = &ring32[(p >> 2) & W4M];
		uint32_t w0, w1, w2;
		if (OWN_AHEAD && S_ >= 128) {         // (the two fetches of the prologue read their own)
			w0 = o1.w0;
			w1 = o1.w1;
			w2 = o1.w2;
		} else {
			w0 = w[0];
			w1 = w[1];
			w2 = w[2];
		}
		f.v = __builtin_amdgcn_alignbyte(w1, w0, p & 3);
		f.vh = __builtin_amdgcn_alignbyte(w2, w1, p & 3);
		const bool can = INNER || p + HD_MIN_MATCH <= n;
		// (a lane past the end of the block publishes nothing; it reads slot 0, harmlessly)
		const uint32_t ha = hash_slot_addr(f.v, hk);             // byte offset of the entry
		uint16_t *const slot = (uint16_t *)((uint8_t *)table + (can ? ha : 0u));
		const uint16_t mine = (uint16_t)(p + 1);
		const uint32_t e = *slot;
		if (can)
			*slot = mine;
		if (INNER) {
			f.c = e;                                         // position + 1 itself: nothing has wrapped
		} else {
			// entry -> absolute position + 1 of the latest p' < p with p' + 1 == e (mod 2^16)
			const uint32_t back = (p + 1 - e) & 0xffffu;         // 0: an entry exactly 2^16 back, i.e. stale
			f.c = (can && e && back) ? p + 1 - back : 0u;
		}
		if (INTRA) {
			// a nearer occurrence inside the step replaces the table's candidate
			const uint32_t d = intra_step_distance<INTRA>(f.v, lane);
			f.c = (can && d) ? p + 1 - d : f.c;
		}
		// Lanes of this step whose four bytes hash alike stored to one entry in that single ds_write_b16:
		// on gfx950 the highest lane's data stays -- the largest position, which is what the CPU twin
		// keeps.  hipdeflate_selftest() checks that property of the LDS on the device (hd_selftest.hip,
		// k_selftest_lds_order), every kernel-vs-twin test leans on it.  (A read-back loop that re-wrote
		// until the slot held the maximum stood here in round 1; the compiler forwarded each lane's own
		// store to its re-read, so it never ran -- and never had to.)
		return f;
	};
	// the three ring dwords under the candidate c (position + 1) of the lane at p.  Neither `spare` nor p is read: they are
	// the shape of the probe of the removed wider geometries, which read ten more dwords here, and the compiler schedules
	// these kernels by it -- without them a few moves trade places in all three.  Kept so that the machine code stays
	// the measured one
	struct Probed {
		uint32_t c0, c1, c2;
		uint32_t spare[10];
	};
	auto probe = [&](uint32_t c, uint32_t p) -> Probed {
		Probed q = {};
		const uint32_t *w = &ring32[((c - 1) >> 2) & W4M];
		q.c0 = w[0];
		q.c1 = w[1];
		q.c2 = w[2];
		return q;
	};

	// ---- the back of the pipeline: codes + bit packing for up to 64 queued tokens
	// (straight-line: both forms computed, one selected); false = the static
	// stream no longer fits under `limit`
	uint32_t qhead = 0, qtail = 0;                                    // TOK: the LDS queue
	// Level 1: the queue is a register.  Lane j of Q0 holds waiting token j, qn of them wait (< 64 at every step's start);
	// a step pushes its tokens across the lanes to [qn, qn + count) mod 64 (queue_push, hd_device.hpp), and when that
	// passes 64 the pass takes Q0 and what wrapped round -- lanes [0, qn + count - 64) of the pushed register -- is the
	// new Q0.  Lanes of Q0 from qn on hold anything
	uint32_t Q0 = 0, qn = 0;
	// What a step pushed joins Q0 one step LATER, behind the next step's probe and fetch have been issued: the push is an
	// LDS-crossbar instruction, and merged where it is issued every step ended on its round trip (s_waitcnt lgkmcnt(0)
	// straight behind the ds_permute_b32).  Now that wait is the one the next fetch makes for its own bytes anyway; only
	// a step that runs the emit pass still waits at once.  Qp: the pushed register, qpm: its lanes that are entries of
	// Q0 (the new ones; all 64 behind a pass, when what wrapped round is the whole queue)
	uint32_t Qp = 0;
	uint64_t qpm = 0;
	auto queue_settle = [&]() {
		Q0 = sel(qpm, Qp, Q0);
		qpm = 0;
	};
	auto count_symbol = [&](uint32_t c) {                             // TOK only
		atomicAdd(&stage[c], 1u);
	};
	// tq: the tokens (level 1; TOK reads its queue)
	auto emit_tokens = [&](uint32_t count, uint32_t tq) -> bool {
		uint32_t t = tq;
		if (TOK) {
			t = tokbuf[(qhead + lane) & (TOKQ - 1)];
			qhead += count;
		}
		if (!use_static)
			return false;                            // given up earlier in this group of steps: nothing more is made
		if (TOK) {
			// queued tokens -> slab (one coalesced 4 B/lane store) + symbol histograms
			if (ntok_slab + count > lay.cap_tok)
				return use_static = false;           // more tokens than the slab holds: the fused kernel's block
			if (lane < count) {
				slab[ntok_slab + lane] = t;
				if (t & HD_TOKEN_MATCH) {
					uint32_t ls, leb, lev, ds, deb, dev;
					len_slot(((t >> 16) & 0xff) + 3, ls, leb, lev);
					off_slot((t & 0xffff) + 1, ds, deb, dev);
					count_symbol(257 + ls);
					count_symbol(286 + ds);
				} else {
					count_symbol(t & 0xff);
				}
			}
			ntok_slab += count;
			return true;
		}
		// literal / length: one table load (CrcTables::SL); offset: slot arithmetic, 5-bit code + extra bits
		// The table gather goes out first, and the staged dwords leave in its shadow: their LDS round trip runs beside
		// the gather's, and their store is issued behind the wait for the gather -- vmcnt counts in issue order, so a
		// store in front of the gather (drain() first, as it was) made that wait stand for the store's round trip too.
		// Behind it, nothing ever waits for the store: the next vector-memory wait is a pass or a refill away
		const uint64_t mmask = __ballot((int32_t)t < 0);
		const uint64_t vmask = count >= 64 ? ~0ull : (1ull << (count & 63)) - 1;
		uint32_t e0 = ct->SL[sel(mmask, (t >> 16) & 0x1ff, t & 0xff)];
		uint32_t ds, deb, dev;
		off_slot((t & 0xffff) + 1, ds, deb, dev);
		uint32_t dpart = (__brev(ds) >> 27) | (dev << 5);
		// (the gather and the offset arithmetic stay in front of the LDS half, the store behind the wait for the gather)
		asm volatile("" : "+v"(dpart), "+v"(deb) : : "memory");
		uint32_t fl;
		const uint32_t dv = drain_read(fl);
		asm volatile("" : "+v"(e0) : : "memory");
		drain_store(fl, dv);
		const uint32_t nb0 = e0 >> 16;
		const uint32_t code = sel(vmask, sel(mmask, (e0 & 0xffff) | (dpart << nb0), e0 & 0xffff), 0u);
		const uint32_t nbits = sel(vmask, sel(mmask, nb0 + 5 + deb, nb0), 0u);
		const uint32_t incl = wave_incl_scan<true>(nbits);
		const uint32_t total = readlane(incl, 63);
		// (in 32 bits: a 64-bit compare of two uniform values is a VECTOR compare on this machine -- v_mov_b64 + v_cmp_gt_u64 per step.
		// limit_bits <= 0xffffff00 and what has passed this test is <= limit_bits, so the sum cannot wrap)
		if ((bitpos - paybase) + total + 7 > limit_bits)
			return use_static = false;
		put(code, nbits, incl, total);
		return true;
	};

	// BFINAL = 1 (0 in flush form), BTYPE = 01
	if (!TOK)
		put(lane == 0 ? (flush ? 2u : 3u) : 0u, lane == 0 ? 3u : 0u, 3u, 3u);

	Fetched f0 = { 0, 0, 0 }, f1 = { 0, 0, 0 };
	Probed q0 = {};
	if (use_static && n) {
		fill_piece();
		f0 = fetch(std::false_type{}, 0);
		q0 = probe(f0.c, lane);
		f1 = fetch(std::false_type{}, 64);
		if (OWN_AHEAD)
			o1 = own(128);
	}
	uint32_t carry = 0;                  // leading positions covered by the last match
	// one step; false = the static stream was abandoned
	// NOFILL: the caller has refilled the ring for this step (the 16-step groups of the main loop)
	// ROOM258: every lane of the step has HD_MAX_MATCH bytes ahead (the groups again), so no long match is clipped by the
	// block's end and the extension's bound is a constant
	auto step = [&](auto inner_tag, auto nofill_tag, auto room258_tag, uint32_t S) -> bool {
		constexpr bool INNER = decltype(inner_tag)::value;
		constexpr bool NOFILL = decltype(nofill_tag)::value;
		constexpr bool ROOM258 = decltype(room258_tag)::value;
		if (!NOFILL && filled < n && filled < S + HD_LOOKAHEAD)
			fill_piece();
		const uint32_t lo = filled > W ? filled - W : 0;
		const uint32_t lanes = INNER ? 64u : (n - S < 64 ? n - S : 64);

		// stage 2 of step k+1 and stage 1 of step k+2 go out first
		const Fetched fc = f0;
		const Probed qc = q0;
		f0 = f1;
		q0 = probe(f1.c, S + 64 + lane);   // harmless beyond n: every index is masked into the ring
		f1 = fetch(inner_tag, S + 128);
		if (OWN_AHEAD)
			o1 = own(S + 192);                 // (every index is masked into the ring; bytes beyond the block never count)
		if (!TOK)
			queue_settle();                    // the last step's tokens (a covered step below pushes none and leaves qpm 0)

		// ---- 3. verify the candidate + first 8 bytes of its length ---------
		// Conditions live as 64-bit lane masks in scalar registers (hd_device.hpp "lane masks"): each is the
		// ballot of ONE compare, they are combined by s_and / s_andn2 and reach the lanes again through sel().
		const uint64_t lanem = (INNER || lanes == 64) ? ~0ull : (1ull << (lanes & 63)) - 1;   // lanes inside the block
		// GROUP (level 1's steps of a group): p is the position + K (lane_k above).  Its readers there are the token word
		// and the long-match events' ring addresses, which are masked; the general steps and the parse kernel, which
		// compare p with the block's end, keep the position itself
		constexpr bool GROUP = !TOK && INNER && ROOM258;
		const uint32_t p = S + (GROUP ? lane_k : lane);
		const uint32_t cv0 = fc.v, cvh0 = fc.vh;
		const uint32_t room = n - p;                  // >= 4 where a match can start
		const uint32_t c = fc.c, cp = c - 1;
		// (v_alignbyte_b32 reads bits [1:0] of its shift operand and no others -- hipdeflate_selftest() checks that on the
		// device -- so the candidate's position goes in whole: no v_and_b32 ..., 3 in front of the pair)
		const uint32_t cv = __builtin_amdgcn_alignbyte(qc.c1, qc.c0, cp);
		const uint32_t cvh = __builtin_amdgcn_alignbyte(qc.c2, qc.c1, cp);
		const uint32_t x = cvh ^ cvh0;
		const uint64_t xm = __ballot(cvh == cvh0);                      // all eight bytes agree
		const uint32_t len8 = sel(xm, 8u, 4u + ((uint32_t)__builtin_ctz(x) >> 3));     // (x == 0: not selected)
		// candidate inside the window (c == 0, no candidate, makes cp = -1: one signed compare covers both;
		// this kernel never sees a block of 2 GiB), its four bytes equal
		uint64_t okm = __ballot((int32_t)cp >= (int32_t)lo) & __ballot(cv == cv0);
		const uint32_t mylen = INNER ? len8 : (len8 < room ? len8 : room);     // <= 8 until a capped match is extended
		if (!INNER)
			okm &= __ballot(p + HD_MIN_MATCH <= n);

		if (carry >= lanes) {                // the whole step lies inside the last match
			carry -= lanes;
			return true;
		}

		// ---- 4. greedy resolution as a wave prefix scan ---------------------
		// The greedy parse is a little automaton walking the lanes: its state
		// r = "lanes still covered by the current match"; a lane with r == 0
		// starts a token and sets r = len - 1 (0 for a literal), otherwise
		// r -= 1.  Each lane's transition f_l : {0..7} -> {0..7} is eight bytes;
		// composing two of them is two v_perm_b32 table lookups, so the state
		// entering every lane comes out of a 6-stage DPP scan -- no per-match
		// serial loop (DNA-like data has ~12 matches per 64 bytes).  Matches
		// whose first 8 bytes all agree ("capped") are rare; when the scan
		// takes one it is extended cooperatively and the scan is redone for
		// the lanes behind it.
		const uint64_t capmask = INNER ? (okm & xm) : (okm & xm & __ballot(room > 8));
		const uint32_t jump8 = sel(okm, mylen, 1u);                  // token length as the scan sees it
		uint32_t lenv = jump8;                                       // ... and with capped matches extended
		const uint64_t livem = ~0ull << carry;                       // lanes the last match does not cover (carry < 64)
		// (token words are prepared here, ahead of the scan: independent work for the wait states between its
		// DPP stages)  match: HD_TOKEN_MATCH_TAG | (len - 3) << 16 | (dist - 1), dist - 1 = p - c
		// (GROUP: the constant is in p already, and the word is one v_sub_u32 here and one v_lshl_add_u32 below)
		const uint32_t mw_base = GROUP ? p - c : (p + (HD_TOKEN_MATCH_TAG - (3u << 16) - 1u)) - cp;
		const uint32_t lit = cv0 & 0xff;
		// K16: length over 16 bytes (valid on the capped lanes).  (The dwords are read here, and the kernel is bound
		// by its instruction count: it skips all of this in a step without a capped lane -- a quarter of the steps on
		// FASTQ-like data.  + 16 mirrored bytes behind the ring: dwords [0,5) of an index never wrap)
		uint32_t len16 = 8;
		const bool k16_step = K16 && capmask != 0;
		if (k16_step) {
			const uint32_t *wp = &ring32[(p >> 2) & W4M], *wc = &ring32[(cp >> 2) & W4M];
			const uint32_t c2 = qc.c2;
			const uint32_t p2 = wp[2], p3 = wp[3], p4 = wp[4];
			const uint32_t c3 = wc[3], c4 = wc[4];
			const uint32_t xa = __builtin_amdgcn_alignbyte(p3, p2, p & 3) ^ __builtin_amdgcn_alignbyte(c3, c2, cp);   // bytes 8..11
			const uint32_t xb = __builtin_amdgcn_alignbyte(p4, p3, p & 3) ^ __builtin_amdgcn_alignbyte(c4, c3, cp);   // bytes 12..15
			// (v_ffbl_b32 of 0 is -1: >> 3 and min 4 turn it into "all four agree"; ka >> 2 is 1 exactly then)
			uint32_t fa, fb;
			asm("v_ffbl_b32 %0, %1" : "=v"(fa) : "v"(xa));
			asm("v_ffbl_b32 %0, %1" : "=v"(fb) : "v"(xb));
			const uint32_t ka = (fa >> 3) < 4 ? (fa >> 3) : 4u, kb = (fb >> 3) < 4 ? (fb >> 3) : 4u;
			len16 = 8 + ka + (ka >> 2) * kb;
			if (!INNER)
				len16 = len16 < room ? len16 : room;
		}
		// K16, continuation lanes.  A capped match of 9..15 bytes at lane m is taken apart for the automaton: m
		// jumps 8, and lane m + 8 -- its "continuation lane" -- jumps the k = len - 8 bytes that are left, whatever
		// candidate that lane has itself.  A parse that takes m arrives at m + 8 with state 0, walks on k lanes and
		// is where the match of 8 + k bytes would have put it: no scalar work at all.  The continuation lane is a
		// token start for the scan only (`v` below: not queued; the token of m carries the whole length).  What
		// is left for the scalar loop: matches of 16 bytes and more (k8m), and continuation lanes the parse reached
		// WITHOUT taking their parent (the parent lies under an earlier token): there the lane's own candidate
		// counts, and the chain is re-threaded from it.  On text that is one event in 12 steps instead of 2.5 per step.
		//   A     parents: capped, 9..15 bytes, not themselves the continuation lane of a parent (stride-8 chains
		//         alternate: A[l] = capk[l] & ~A[l - 8])
		//   contm continuation lanes (A << 8; a parent in lanes 56..63 has none: its token simply ends in the next step)
		//   jumpA what the automaton sees, jumpW the true length of a token that starts at the lane (16+: 8 for now)
		uint64_t k8m = 0, par = 0, contm = 0;
		uint32_t jumpA = jump8, jumpW = jump8;
		if (k16_step) {
			k8m = capmask & __ballot(len16 == 16);
			const uint64_t capk = capmask & ~k8m & __ballot(len16 != 8);
			par = capk;
			if (capk & (capk << 8)) {
#pragma unroll
				for (int i = 0; i < 7; i++)
					par = capk & ~(par << 8);
			}
			contm = (par << 8) & lanem;
			const uint32_t kc = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane - 8) << 2), (int)(len16 - 8));
			jumpW = sel(capk, len16, jump8);
			jumpA = sel(contm, kc, jump8);
			lenv = jumpW;
		}
		uint64_t starts;
		{
			// fn8_make: {a, 0, 1, 2 | 3, 4, 5, 6} with a = jump - 1; the lanes the last match covers are literals
			// (a = 0), not the identity: state 0 enters lane 0 and a literal hands it on, so the first live lane sees
			// 0 either way and livem masks the covered lanes' own "starts" below.  Every map being elementary, the
			// upper dword is one constant for the wave and the scan's first three stages know theirs (Fn8Ident)
			Fn8 f;
			f.lo = sel(livem, jumpA + 0x0200ffffu, 0x02010000u);
			f.hi = 0x06050403u;
			const uint32_t w0 = fn8_scan_state0(f, fid, fcross);
			// state entering lane l = (f_{l-1} o ... o f_0)(0): byte 0 of lane l-1, and 0 enters lane 0 -- the mask of
			// "a state other than 0 behind the lane", one lane up, in scalar registers: the shift brings in the 0 that
			// lane 0 wants, and the NOT is the s_andn2 that applies livem (a wave_shr:1 of the bytes in front of the
			// compare is a vector instruction and two wait states)
			starts = livem & ~(__ballot((w0 & 0xff) != 0) << 1);
		}
		// Capped matches the scan took: extend each (left to right) to its true
		// length, drop the token starts it now covers, and re-thread the chain
		// behind it.  Two parses that start a token on the same lane coincide
		// from there on, so the walk stops at the first old start it lands on
		// (a few hops) instead of re-scanning the wave.
		uint64_t v = 0;                      // K16: continuation lanes whose parent the parse took
		if (K16) {
			uint64_t pend = ~0ull;           // lanes behind the last event
			for (;;) {
				v = starts & contm & ((starts & par) << 8);
				const uint64_t ev = starts & (k8m | contm) & ~v & pend;
				if (!ev)
					break;
				const uint32_t m = (uint32_t)__ffsll((unsigned long long)ev) - 1;
				uint32_t len;
				if ((k8m >> m) & 1) {
					// 16 bytes and more: extended as below, from byte 16 on
					const uint32_t pm = S + m;
					const uint32_t dm = pm + 1 - readlane(c, m);
					const uint32_t maxlen = n - pm < HD_MAX_MATCH ? n - pm : HD_MAX_MATCH;
					uint32_t t0, t1, k;
					len = 16;
					asm volatile("Lhd_ext_%=:\n\t"
					     "v_add_u32 %[t0], %[len], %[vb]\n\t"
					     "v_add_u32 %[t1], %[ndm], %[t0]\n\t"
					     "v_and_or_b32 %[t0], %[t0], %[msk], %[rb]\n\t"
					     "v_and_or_b32 %[t1], %[t1], %[msk], %[rb]\n\t"
					     "ds_read_u8 %[t0], %[t0]\n\t"
					     "ds_read_u8 %[t1], %[t1]\n\t"
					     "s_waitcnt lgkmcnt(0)\n\t"
					     "v_cmp_ne_u16 vcc, %[t0], %[t1]\n\t"
					     "s_cbranch_vccnz Lhd_ext_hit_%=\n\t"
					     "s_add_u32 %[len], %[len], 64\n\t"
					     "s_cmp_lt_u32 %[len], %[maxlen]\n\t"
					     "s_cbranch_scc1 Lhd_ext_%=\n\t"
					     "s_branch Lhd_ext_done_%=\n"
					     "Lhd_ext_hit_%=:\n\t"
					     "s_ff1_i32_b64 %[k], vcc\n\t"
					     "s_add_u32 %[len], %[len], %[k]\n"
					     "Lhd_ext_done_%=:"
					     : [len] "+s"(len), [t0] "=&v"(t0), [t1] "=&v"(t1), [k] "=&s"(k)
					     : [vb] "v"(pm + lane), [ndm] "s"(0u - dm), [msk] "s"(W - 1), [rb] "v"(ring_lds), [maxlen] "s"(maxlen)
					     : "vcc", "scc", "memory");
					len = len < maxlen ? len : maxlen;
					// (v_writelane_b32 with the lane select in M0: the one form that may name two scalar operands on
					// gfx9.  Nothing else in this kernel uses M0 -- LDS instructions do not need it here)
					asm("s_mov_b32 m0, %2\n\ts_nop 0\n\tv_writelane_b32 %0, %1, m0" : "+v"(lenv) : "s"(len), "s"(m));
				} else {
					len = readlane(jumpW, m);            // a continuation lane on its own: its own candidate (or a literal)
				}
				// re-thread behind the token of m.  The old chain is good again from its first start that is not a
				// continuation lane (those behave differently when they are reached from elsewhere)
				uint64_t fresh = 0;
				// (the merge of an asm result and a v_readlane counts as divergent for the compiler: pinned)
				uint32_t xq = m + (uint32_t)__builtin_amdgcn_readfirstlane((int)len), hop;
				asm volatile("s_cmp_gt_u32 %0, 63\n\t"
					     "s_cbranch_scc1 Lhd_rethread_done_%=\n"
					     "Lhd_rethread_%=:\n\t"
					     "s_bitcmp1_b64 %3, %0\n\t"
					     "s_cbranch_scc1 Lhd_rethread_done_%=\n\t"
					     "s_bitset1_b64 %1, %0\n\t"
					     "v_readlane_b32 %2, %4, %0\n\t"
					     "s_add_u32 %0, %0, %2\n\t"
					     "s_cmp_lt_u32 %0, 64\n\t"
					     "s_cbranch_scc1 Lhd_rethread_%=\n"
					     "Lhd_rethread_done_%=:"
					     : "+s"(xq), "+s"(fresh), "=&s"(hop)
					     : "s"(starts & ~contm), "v"(jumpW)
					     : "scc");
				const uint32_t xe = xq < 64 ? xq : 64;
				uint64_t gone;                           // lanes (m, xe): xe - m - 1 may be 0 here (a literal at m)
				asm("s_bfm_b64 %0, %1, %2" : "=s"(gone) : "s"(xe - m - 1), "s"(m + 1));
				starts = (starts & ~gone) | fresh;
				pend = ~1ull << m;
			}
		} else {
			// The long-match events of the step: one block of assembly, run once per event.  (The loop around it is the
			// compiler's, s_cmp_lg_u64 + branch on the block's last result: an asm goto with scalar outputs, which
			// would let the block branch on the SCC of its own last AND, crashes this compiler's instruction selection.)
			//   todo   the capped lanes no event has handled yet.  An event clears its own bit, and that is all the
			//          bookkeeping there is: the events run in rising lane order, fresh starts lie behind the match
			//          that made them, and a lane below the last event is a start now iff it was one then -- so
			//          starts & todo is "the capped starts above m": the AND at the block's bottom is the loop test
			//   m      lives in M0 from the s_ff1_i32_b64 on: s_bitset0_b64, s_add, s_sub, v_readlane_b32 and
			//          v_writelane_b32 all take it there (v_writelane_b32 with the lane select in M0 is the one form
			//          that may name two scalar operands on gfx9).  Nothing else in this kernel uses M0 -- LDS
			//          instructions do not need it here
			//   x      m + length so far: the scalar half of the step-relative address (p = S + lane is the vector
			//          half, so no per-event vector add forms pm + lane), and the walk's first lane when the
			//          extension ends.  The candidate's side is cq = (c - 1 of lane m) + length so far + lane
			//   extension  64 bytes per pass, every index masked into the ring.  The passes compare bytes 2..65,
			//          66..129, 130..193 and 194..257 of the match (the first eight are known to agree; the 2 is the
			//          candidate read's offset and the first x, and the ring's 16 mirrored bytes cover it): the last
			//          pass ends on byte 257, so a mismatch found in any pass is a length below 258 and the
			//          no-hit exit is 258 itself -- ROOM258 needs no clamp at all.  A step that is not ROOM258 cuts
			//          both exits to the bytes the block has left (lanes past them may read too)
			//   len == 8   (one event in six) takes the same path: lane m + 8 is an old start or lies behind the step, so
			//          the walk ends where it begins and `gone` holds no start.  An exit of its own -- a compare and a
			//          branch in every event -- measured slower
			//   the walk   re-threads the chain behind the match: lanes it lands on become starts (fresh) until it
			//          lands on an old start -- two parses that start a token on one lane coincide from there on -- or
			//          leaves the step.  It reads lenv: behind the match no event has touched it yet.  The lane
			//          selects of v_readlane / s_bitcmp1 / s_bitset1 take the low 6 bits and x < 64 is tested first;
			//          an SGPR written by the SALU needs no wait states before v_readlane uses it as lane select
			//   gone   the old starts in (m, x): one s_bfm_b64 of min(x, 64) - m - 1 ones from bit m + 1 (m == 63
			//          makes it empty)
			//   ring   THE RING IS THE KERNEL'S FIRST LDS OBJECT, at LDS address 0: it has the largest alignment (W), and
			//          the objects are laid out by falling alignment.  So the ring address of an index is the index AND
			//          W - 1 and nothing else -- v_and_b32 with a literal, VOP2 -- where the general form
			//          (x & (W - 1)) | base is a VOP3 with a scalar source, in the dearer class, OR-ing in a zero.
			//          Stated here and nowhere else; tests/test_l1_trim_isa.py holds the layout by the listing (the
			//          table's accesses carry offset:W + 16).  The parse kernel's K16 loop above keeps the general form
			uint64_t todo = capmask;
			uint64_t cm = starts & todo;
			if (cm) {
				uint32_t t0, t1, x, cq, len, k;
				uint64_t fresh;
#define HD_L1_EVENTS(CLAMP)                                                                  \
	"s_ff1_i32_b64 m0, %[cm]\n\t"                                                        \
	"s_bitset0_b64 %[todo], m0\n\t"                                                      \
	"v_readlane_b32 %[cq], %[cp], m0\n\t"                                                \
	"s_add_u32 %[x], m0, 2\n"                                                            \
	"Lhd_ext_%=:\n\t"                                                                    \
	"v_add_u32 %[t0], %[x], %[p]\n\t"                                                    \
	"v_add_u32 %[t1], %[cq], %[lane]\n\t"                                                \
	"v_and_b32 %[t0], %[wm], %[t0]\n\t"                                                  \
	"v_and_b32 %[t1], %[wm], %[t1]\n\t"                                                  \
	"ds_read_u8 %[t0], %[t0]\n\t"                                                        \
	"ds_read_u8 %[t1], %[t1] offset:2\n\t"                                               \
	"s_waitcnt lgkmcnt(0)\n\t"                                                           \
	"v_cmp_ne_u16 vcc, %[t0], %[t1]\n\t"                                                 \
	"s_cbranch_vccnz Lhd_ext_hit_%=\n\t"                                                 \
	"s_add_u32 %[x], %[x], 64\n\t"                                                       \
	"s_add_u32 %[cq], %[cq], 64\n\t"                                                     \
	"s_sub_u32 %[len], %[x], m0\n\t"                                                     \
	"s_cmp_lt_u32 %[len], 258\n\t"                                                       \
	"s_cbranch_scc1 Lhd_ext_%=\n\t"                                                      \
	"s_branch Lhd_ext_len_%=\n"                                                          \
	"Lhd_ext_hit_%=:\n\t"                                                                \
	"s_ff1_i32_b64 %[k], vcc\n\t"                                                        \
	"s_add_u32 %[x], %[x], %[k]\n\t"                                                     \
	"s_sub_u32 %[len], %[x], m0\n"                                                       \
	"Lhd_ext_len_%=:\n\t"                                                                \
	CLAMP                                                                                \
	"v_writelane_b32 %[lenv], %[len], m0\n\t"                                            \
	"s_mov_b64 %[fresh], 0\n\t"                                                          \
	"s_cmp_gt_u32 %[x], 63\n\t"                                                          \
	"s_cbranch_scc1 Lhd_rethread_out_%=\n"                                               \
	"Lhd_rethread_%=:\n\t"                                                               \
	"s_bitcmp1_b64 %[starts], %[x]\n\t"                                                  \
	"s_cbranch_scc1 Lhd_rethread_done_%=\n\t"                                            \
	"s_bitset1_b64 %[fresh], %[x]\n\t"                                                   \
	"v_readlane_b32 %[k], %[lenv], %[x]\n\t"                                             \
	"s_add_u32 %[x], %[x], %[k]\n\t"                                                     \
	"s_cmp_lt_u32 %[x], 64\n\t"                                                          \
	"s_cbranch_scc1 Lhd_rethread_%=\n"                                                   \
	"Lhd_rethread_out_%=:\n\t"                                                           \
	"s_movk_i32 %[x], 64\n"                                                              \
	"Lhd_rethread_done_%=:\n\t"                                                          \
	"s_add_u32 %[k], m0, 1\n\t"                                                          \
	"s_sub_u32 %[len], %[x], %[k]\n\t"                                                   \
	"s_bfm_b64 %[cm], %[len], %[k]\n\t"                                                  \
	"s_andn2_b64 %[starts], %[starts], %[cm]\n\t"                                        \
	"s_or_b64 %[starts], %[starts], %[fresh]\n"                                          \
	"s_and_b64 %[cm], %[starts], %[todo]"
				do {
					if (ROOM258)
						asm volatile(HD_L1_EVENTS("")
						  : [starts] "+s"(starts), [todo] "+s"(todo), [cm] "+s"(cm), [lenv] "+v"(lenv), [t0] "=&v"(t0), [t1] "=&v"(t1),
						    [x] "=&s"(x), [cq] "=&s"(cq), [len] "=&s"(len), [k] "=&s"(k), [fresh] "=&s"(fresh)
						  : [cp] "v"(cp), [p] "v"(p), [lane] "v"(lane), [wm] "n"(W - 1)
						  : "vcc", "scc", "memory");
					else
						asm volatile(HD_L1_EVENTS("s_sub_u32 %[k], %[left], m0\n\t"
								       "s_min_u32 %[k], %[k], 258\n\t"
								       "s_min_u32 %[len], %[len], %[k]\n\t"
								       "s_add_u32 %[x], %[len], m0\n\t")
						  : [starts] "+s"(starts), [todo] "+s"(todo), [cm] "+s"(cm), [lenv] "+v"(lenv), [t0] "=&v"(t0), [t1] "=&v"(t1),
						    [x] "=&s"(x), [cq] "=&s"(cq), [len] "=&s"(len), [k] "=&s"(k), [fresh] "=&s"(fresh)
						  : [cp] "v"(cp), [p] "v"(p), [lane] "v"(lane), [wm] "n"(W - 1), [left] "s"(n - S)
						  : "vcc", "scc", "memory");
				} while (cm);
#undef HD_L1_EVENTS
			}
		}
		// coverage behind the last token of the step
		// (the last REAL start: a continuation lane behind it belongs to its token)
		// != 0: carry < lanes, and the first start is real -- so level 1 takes the bare s_flbit_i32_b64 (__clzll also answers
		// for 0: an s_min_u32 ..., 64 behind it in every step)
		const uint64_t real = starts & ~v;
		// Level 1: last - 64 = ~clz (63 - clz - 64), and v_readlane_b32 takes the low six bits of its lane select, which
		// are last's: E - 64 comes out of the add, and the carry is ONE signed max below
		const uint32_t last = K16 ? 63 - (uint32_t)__clzll((long long)real) : ~(uint32_t)__builtin_clzll(real);
		const uint32_t E = last + readlane(lenv, last);              // K16: the end of the last token; level 1: that - 64
		const uint64_t tm = starts & lanem & ~v;           // tokens: matches + literals inside the block
		const uint64_t mm = tm & okm;                      // matches
		// max(E, 64) - 64 in scalar registers (written in C the compiler makes a v_sub ... clamp + v_readfirstlane of
		// it); tail step: matches are clipped to n
		if (!(INNER || lanes == 64))
			carry = 0;
		else if (K16)
			asm("s_max_u32 %0, %1, 64\n\ts_sub_u32 %0, %0, 64" : "=s"(carry) : "s"(E) : "scc");
		else
			asm("s_max_i32 %0, %1, 0" : "=s"(carry) : "s"(E) : "scc");

		// ---- 5. queue the step's tokens in position order -------------------
		// token word: literal byte, or HD_TOKEN_MATCH_TAG | (len - 3) << 16 | (dist - 1), dist - 1 = p - c.
		// The code generation and the bit packing below cost the same for 1 or 64
		// tokens, and DNA-like input yields only ~14 tokens per step: they wait in
		// a queue (TOK: a small LDS ring; level 1: a register) until 64 are there.
		// (a failed pass -- the stream would pass `limit`, or the slab is full -- clears use_static and the
		// passes after it do nothing: the steps of a group need no exits between them)
		const uint32_t tw = sel(mm, (lenv << 16) + mw_base, lit);
		if (TOK) {
			const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(tm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)tm, 0));
			const uint32_t qslot = (qtail + rank) & (TOKQ - 1);
			if ((tm >> lane) & 1)
				tokbuf[qslot] = tw;
			qtail += (uint32_t)__popcll(tm);
			db_room -= (int32_t)__popcll(tm);
			if (qtail - qhead >= 64)
				emit_tokens(64, 0);
		} else {
			const uint32_t R = queue_push(tm, qn, tw);
			uint64_t newm;                                   // lanes qn..63 (lanes behind the step's last token take whatever came: not yet entries)
			asm("s_lshl_b64 %0, -1, %1" : "=s"(newm) : "s"(qn) : "scc");
			Qp = R;
			qpm = newm;
			qn += (uint32_t)__popcll(tm);
			if (qn >= 64) {
				emit_tokens(64, sel(newm, R, Q0));
				qpm = ~0ull;                             // Q0 = R, one step on
				qn -= 64;
			}
		}
		return use_static;
	};
	// fetch runs two steps ahead: a step is INNER when the lanes of step S + 128 still have 9 bytes
	// (<= 2^16: the last position that enters the table is n - 4, so position + 1 still fits the
	// 16-bit entries of a block of exactly 0x10000 bytes -- the reference's single-thread block size, applet/7bgzf.c:146-147.
	// Such blocks had been running through the general steps: 244 GB/s against 323 for 0xff00-byte blocks, which rounds 1-2
	// took for HBM channel aliasing; a start stagger of the waves, tried on that theory, only cost time.)
	const bool small = n <= 65536;
	// TOK: the open DEFLATE block's histograms leave for HBM and start again from zero
	auto close_deflate_block = [&]() {
		uint32_t *h = (uint32_t *)(rec + lay.off_hist) + ndb * 320;
		// HBM layout: u32 litlen [0,288), offset [288,320)
		for (uint32_t i = lane; i < 320; i += 64) {
			const uint32_t j = i < 286 ? i : i - 2;          // counter of litlen i / offset i - 288
			const bool used = i < 286 || (i >= 288 && i < 318);
			h[i] = used ? stage[j] : 0u;
		}
		for (uint32_t i = lane; i < 316u; i += 64)
			stage[i] = 0;
		if (lane == 0)
			((uint32_t *)(rec + lay.off_ntok))[ndb] = ntok_slab - db_start;
		db_start = ntok_slab;
		db_room = HD_DYN_BLOCK_TOKENS;
		ndb++;
	};
	// a DEFLATE block closes at the first step boundary with >= 32768 tokens (as the fused kernel)
	// (db_room == HD_DYN_BLOCK_TOKENS - (ntok_slab + queued - db_start); an INNER step is never the last one)
	auto step_boundary = [&](auto inner_tag, uint32_t S) -> bool {
		constexpr bool INNER = decltype(inner_tag)::value;
		if (TOK && db_room <= 0 && use_static && (INNER || S + 64 < n)) {
			if (qtail != qhead && !emit_tokens(qtail - qhead, 0))
				return false;
			close_deflate_block();
		}
		return use_static;
	};
	// The ring is refilled one 1 KiB piece at a time, in the step that would otherwise run out of lookahead:
	// S = 704, 1728, ... (filled == S + 320).  From there the next 16 steps need no refill, and while all
	// of them are INNER steps they run as one GROUP: the refill once, then 4 x 4 steps unrolled, so that the
	// three-stage pipeline's hand-over (f0 <- f1 <- fetch, q0 <- probe) is register renaming instead of a
	// dozen v_mov per step, and the refill test and its merge copies leave the steps.
	uint32_t S = 0;
	clk.mark(0);                                 // (diagnostic build only) prologue done
	// priming steps (latency mode, HD_LAT_PRIME): the front of the pipeline only -- the positions enter the table, the ring
	// fills -- and no tokens: the twin drops them, and no match crosses the border.  (A loop of its own, ahead of the main
	// one: inside it the same lines cost the level-1 kernel 0.8 % of its 16 GiB rate.)
	for (; S < prime && use_static; S += 64) {
		if (filled < n && filled < S + HD_LOOKAHEAD)
			fill_piece();
		f0 = f1;
		q0 = probe(f1.c, S + 64 + lane);
		f1 = fetch(std::false_type{}, S + 128);
		if (OWN_AHEAD)
			o1 = own(S + 192);
	}
	while (S < n && use_static) {
		// (... and, for ROOM258, the last lane of its last step has a full match length ahead: 1281 bytes from S on, where
		// INNER alone asks for 1160.  The last group of a 0xff00-byte block fails both)
		if (small && filled < n && filled < S + HD_LOOKAHEAD && S + 15 * 64 + 63 + HD_MAX_MATCH <= n) {
			fill_piece();
#pragma unroll 1
			for (uint32_t g = 0; g < 4 && use_static; g++) {
#pragma unroll
				for (uint32_t u = 0; u < 4; u++) {
					step(std::true_type{}, std::true_type{}, std::true_type{}, S);
					step_boundary(std::true_type{}, S);
					S += 64;
				}
			}
			continue;
		}
		const bool ok_step = (small && S + 192 + 8 <= n) ? step(std::true_type{}, std::false_type{}, std::false_type{}, S)
								  : step(std::false_type{}, std::false_type{}, std::false_type{}, S);
		if (!ok_step || !step_boundary(std::false_type{}, S))
			break;
		S += 64;
	}
	if (TOK && use_static && qtail != qhead)
		emit_tokens(qtail - qhead, 0);
	if (!TOK)
		queue_settle();
	if (!TOK && use_static && qn)
		emit_tokens(uniform(qn), Q0);            // the short last pass (pinned: behind the loops the compiler takes the count for divergent)
	clk.mark(1);                                 // steps done

	// the CRC needs every piece, also when the static stream was abandoned
	while (filled < n) {
		const uint32_t piece = filled / HD_PIECE;
		const uint4 pv = pre;
		filled += HD_PIECE;
		// (here the next piece IS needed at once, by the next pass of this loop: requested first, its round trip
		// and the gathers' overlap; behind them, as in fill_piece, the two would add up)
		if (filled < n)
			pre = load_slot(src, n, piece + 1, lane, aligned);
		crc.fold(ct, piece, piece * HD_PIECE + lane * 16 + 16 <= n && piece * HD_PIECE + lane * 16 >= prime, pv);
	}
	const uint32_t crcv = crc.finish(ct, lane, n, src + (n & ~15u));
	clk.mark(2);                                 // CRC done

	if (TOK) {
		if (use_static)
			close_deflate_block();
		if (lane == 0) {
			uint32_t *m = (uint32_t *)(rec + lay.off_rec);
			m[0] = use_static ? ndb : 0xffffffffu;       // use_static false here: the slab overflowed
			m[1] = crcv;
			if (!parted)                                 // (a part's slab holds a token per byte)
				a.split_ovf[b] = use_static ? 0u : 1u;
		}
		return;
	}
	if (use_static && (uint64_t)(bitpos - paybase) + 7 > 8ull * limit)
		use_static = false;
	if (!use_static) {
		write_stored_member(a, b, src_own, n_own, crcv, lane);
		return;
	}

	// end-of-block (7 zero bits), pad to a byte, then CRC32 + ISIZE as 4 x 16 bits
	bitpos += 7;
	drain();                                     // the tail adds at most four dwords to the one that stays
	if (flush) {
		// header of an empty stored block (BFINAL = 0, BTYPE = 00), alignment, LEN = 0, NLEN = ffff
		bitpos = (bitpos + 3 + 7) & ~7u;
		uint32_t tcode = 0, nb = 0;
		if (lane < 2) {
			tcode = lane ? 0xffffu : 0u;
			nb = 16;
		}
		const uint32_t incl = wave_incl_scan<true>(nb);
		put(tcode, nb, incl, 32);
	}
	bitpos = (bitpos + 7) & ~7u;
	const uint32_t paylen = (bitpos - paybase) >> 3;
	if (trl) {
		uint32_t tcode = 0, nb = 0;
		if (lane < trl / 2) {
			tcode = frame_trl_field(a.frame, lane, crcv, n_own);
			nb = 16;
		}
		const uint32_t incl = wave_incl_scan<true>(nb);
		put(tcode, nb, incl, 8 * trl);
	}
	// final flush: everything left, including the last partial dword (a handful)
	for (uint32_t i = flushed + lane; i < ((bitpos + 31) >> 5); i += 64)
		dst32[i] = stage[i & (STG - 1)];
	if (lane == 0) {
		const uint32_t total = hdr + paylen + trl;
		if (a.frame == HD_FRAME_BGZF)
			*(uint16_t *)((uint8_t *)dst32 + 16) = (uint16_t)(total - 1);
		else if (a.frame == HD_FRAME_MIGZ)
			dst32[4] = paylen;
		a.out_len[b] = total;
		if (a.status) a.status[b] = 0;
		if (a.crc) a.crc[b] = crcv;
	}
}

} // namespace hd
