/*
 * hipdeflate.h -- C ABI of libhipdeflate.so: the MI355X (gfx950) block-parallel
 * DEFLATE engine that sits behind 7bgzf's codec boundary as BGZF_METHOD=hip.
 *
 * Plain C: pointers and sizes only.  Every entry point names the reference
 * interface it replaces or extends (paths relative to cielavenir/7bgzf):
 *
 *   hip_deflate / hip_inflate      = one more backend pair with the
 *       zlibutil_code_enc / zlibutil_code_dec signatures, lib/zlibutil.h:46-47,
 *       next to libdeflate_deflate / libdeflate_inflate (lib/zlibutil.h:101-114,
 *       lib/zlibutil.c:179-204).  DEFLATE_HIP extends the enum at
 *       lib/zlibutil.h:13-26.
 *   bgzf_compress                  = the LD_PRELOAD hook, bgzf_compress.c:39,
 *       with BGZF_METHOD=hip<level> added to its method table (:53-113).
 *   hipdeflate_batch_*             = the batch-shaped form of the per-block
 *       loop of applet/7bgzf.c:159-277 / applet/7migz.c:130-244 (encode) and
 *       applet/7bgzf.c:306-360 (decode): thousands of independent blocks per
 *       call instead of one pthread per block.  No reference counterpart
 *       exists; INTEGRATION.md shows the loop rewritten on top of them.
 *
 * Return convention everywhere: 0 = success, non-zero = failure, as the
 * reference's codecs (applet/7bgzf.c:228-254,350-353 only print the value).
 * There is NO CPU fallback: without a usable gfx950 device every entry point
 * fails (HD_E_NODEVICE) and says so on stderr.
 */
#ifndef HIPDEFLATE_H
#define HIPDEFLATE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* value to add after DEFLATE_KZIP in lib/zlibutil.h:13-26 */
#define DEFLATE_HIP 11

/* library error codes (positive; never collide with the 0..3 inflate codes) */
#define HD_E_NODEVICE  100   /* no HIP device / not gfx950 / runtime error     */
#define HD_E_ARG       101   /* bad argument (alignment, sizes)                 */
#define HD_E_NOMEM     102   /* device or pinned allocation failed              */

/* container framing the encode kernel writes around each payload */
#define HD_FRAME_RAW   0     /* raw DEFLATE only (what a zlibutil codec returns) */
#define HD_FRAME_BGZF  1     /* applet/7bgzf.c:263-272: 18 B header, CRC32, ISIZE */
#define HD_FRAME_MIGZ  2     /* applet/7migz.c:224-233: 20 B header, CRC32, ISIZE */
#define HD_FRAME_RAW_FLUSH 3 /* raw DEFLATE in full-flush form: no block is final, then an empty stored
                              * block header, byte alignment and 00 00 ff ff -- byte for byte what
                              * zlibutil_buffer_full_flush (applet/7dictzip.c:93-126, 7razf.c:126-160)
                              * makes of a codec's output by re-inflating it with a patched zlib; here it
                              * comes straight from the kernel.  Chunks in this form concatenate. */
#define HD_FRAME_ZLIB  4     /* RFC 1950 as zlibutil_buffer_code writes it (lib/zlibutil.c:374-397):
                              * 78 da, raw DEFLATE, Adler-32 big-endian -- the Adler-32 comes from the kernel */
#define HD_FRAME_GZIP  5     /* RFC 1952 as lib/zlibutil.c:379-405: 1f 8b 08 00 <mtime = 0> 02 00, raw
                              * DEFLATE, CRC32, ISIZE (the reference stamps time(NULL); a batch has no clock) */

/* OR'ed into `frame`: LATENCY MODE for batches far smaller than the machine -- what bgzf_compress, hip_deflate and
 * hip_deflate_flush use (one block per call, bgzf_compress.c:163-169, lib/zlibutil.c:179-192).
 *   levels 1..2  every block longer than 4080 (level 1) / 8160 (level 2) bytes is coded as independent flushed segments of
 *                that size, one wavefront each (level 2: four parse wavefronts per segment, HD_LAT_PART_BYTES), stitched on
 *                the device (hipdeflate_params.h HD_LAT_SEG_BYTES): a 0xff00-byte block in about a tenth of one wavefront's
 *                time.  The bytes differ from the throughput form (both are what the CPU twin gives for the same mode).
 *   levels 3..9  ONE CODEC PER LEVEL (round 5; as the reference has, deflate_compress.c:3951-3955): the flag changes the
 *                schedule, not the stream -- the workgroup parse on the whole block and, for blocks up to 64 KiB, the member
 *                written by a workgroup of sixteen wavefronts (hd_emit_wg.hpp) instead of by one; byte for byte the
 *                throughput form's output. */
#define HD_FRAME_LATENCY 0x100

/* ---- lifetime ---------------------------------------------------------- */

/* The device list (SURVEY.md 8(b) `hipdeflate_init(devices...)`; the reference's analogue is -@ N worker threads,
 * applet/7bgzf.c:155-217).  The library keeps one context -- stream, tables, scratch -- per ENTRY of the list; an entry
 * is a HIP device ordinal and an ordinal may be listed twice (two independent contexts on one card: how the
 * multi-device hosts are rehearsed on a one-GPU box).  The list is fixed by the first of:
 *   hipdeflate_init_devices(list, n)            an explicit list (n <= 32);
 *   hipdeflate_init(device)                     device >= 0: a list of one;
 *   hipdeflate_init(-1), or any other entry     HIPDEFLATE_DEVICES=0,1,2,... if set (a list), else a list of one:
 *   point, lazily                               HIPDEFLATE_DEVICE, else LOCAL_RANK (a torch.distributed / RCCL rank owns
 *                                               one card), else 0.
 * Contexts are created on first use.  A thread's calls run on entry 0 unless it chose another with
 * hipdeflate_use_device(index) (thread-local, like hipSetDevice); pipes and latency contexts stay on the entry they
 * were opened on whatever thread calls them; the LD_PRELOAD hook and the per-block codecs spread their batch contexts
 * over the whole list.  Idempotent; hipdeflate_init_devices with a list other than the one in force is HD_E_ARG. */
int  hipdeflate_init(int device);
int  hipdeflate_init_devices(const int *devices, int n);
int  hipdeflate_device_count(void);          /* entries of the list (configures it from the environment if need be) */
int  hipdeflate_use_device(int index);       /* 0, or HD_E_ARG / HD_E_NODEVICE; index = position in the list */
void hipdeflate_shutdown(void);              /* every context; the next call configures the list afresh */
/* 0 if a usable device is present and the kernels loaded, else HD_E_NODEVICE */
int  hipdeflate_available(void);
/* human-readable build/device description, never NULL */
const char *hipdeflate_version(void);
/* Workgroups of the parse kernel (levels >= 3) that have given a block up since the contexts were made, over all contexts: a
 * table turn that did not come within ~40 ms of polling (a preempted or single-stepped device) -- such a block is written
 * STORED: valid, status 0, but not the bytes an undisturbed run writes.  Also counted: an emit wavefront that waited 2 s for a block's
 * parse where the emit kernel runs beside the parse (launches of 512 and more blocks of up to 2 MiB at levels >= 3: the two kernels
 * need to run at the same time, on a stream of the lowest priority class the library makes for it; HIPDEFLATE_NO_BESIDE=1 turns the
 * scheme off) -- the same consequence.  0 in every healthy run; bench.py, the GPU tests and the fuzz tools assert it.
 * (Synchronises the devices.) */
uint64_t hipdeflate_stall_count(void);

/* ---- per-block codecs: drop-in zlibutil backends ------------------------ */

/* zlibutil_code_enc (lib/zlibutil.h:47).  *destLen in = capacity, out = bytes.
 * Output is raw DEFLATE ending in a BFINAL block.  Levels (include/hipdeflate_params.h): 0 stored; 1 greedy + static Huffman
 * (the speed level); 2 greedy + dynamic Huffman in one wavefront's 4 KiB window; 3..9 the workgroup parse -- a 32 KiB window and a
 * 64 KiB multi-way table shared by a workgroup, block splitting -- with 1 way greedy (3), 1 way lazy (4), 2 ways (5), 4 ways (6..9):
 * level 3 is below the reference's libdeflate level 1 in size on every measured set, level 6 within 3 % of its level 6 -- through
 * every entry point: the per-call forms here and the hook write the batch calls' bytes at levels >= 3 (HD_FRAME_LATENCY above).
 * As libdeflate_deflate (lib/zlibutil.c:179-192) a call succeeds whenever the stream fits the room, also for a block longer than the
 * room (applet/7png.c:112 gives 1.5 x the OLD compressed size).  One exception: hipdeflate_batch_deflate_dev at levels >= 3, where only
 * the device knows the lengths and the parse's records are sized by the slot, refuses (status != 0) a block longer than its slot.
 * Re-entrant and thread-safe; concurrent callers whose room covers the latency form's worst case and the stored form share launches
 * (the hook's micro-batcher, an engine per level and frame; HIPDEFLATE_CODEC_BATCH=0: a context per call). */
int hip_deflate(unsigned char *dest, size_t *destLen,
		const unsigned char *source, size_t sourceLen, int level);

/* zlibutil_code_dec (lib/zlibutil.h:46).  Stops at BFINAL, ignores trailing
 * source bytes (applet/7bgzf.c:328 passes payload + 8-byte trailer).  Returns
 * enum libdeflate_result values 0/1/3 like libdeflate_inflate
 * (lib/zlibutil.c:194-204).  Re-entrant and thread-safe, and built for the way the reference calls it -- a thread
 * per block, -@ N at once (applet/7bgzf.c:330-345): concurrent calls are coalesced into one launch (one wavefront
 * per stream, the whole window in LDS) on pinned batch memory, no process-wide lock; the batches are spread over the
 * device list.  At most HIPDEFLATE_INFLATE_INFLIGHT (2) batches are on the device, the collecting one grows meanwhile;
 * HIPDEFLATE_INFLATE_WINDOW_US (400) / _LINGER_US (60) bound how long a batch's first caller waits for the others
 * once a launch slot is free (a lone caller never waits). */
int hip_inflate(unsigned char *dest, size_t *destLen,
		const unsigned char *source, size_t sourceLen);

/* hip_deflate followed by zlibutil_buffer_full_flush (applet/7dictzip.c:93-126):
 * same contract, output in HD_FRAME_RAW_FLUSH form. */
int hip_deflate_flush(unsigned char *dest, size_t *destLen,
		      const unsigned char *source, size_t sourceLen, int level);

/* The decoder for such chunks -- the role zlib_inflate / igzip_inflate play in the
 * readers of 7dictzip (applet/7dictzip.c:318-323) and 7razf: a chunk has no final
 * block, so the stream may also stop after a non-final block once every source byte
 * has been used (lib/zlibutil.c:289-291, lib/zlibutil_igzip.c:111: "out of input" is
 * success there).  Input that runs out inside a block is still HD_BAD_DATA. */
int hip_inflate_flush(unsigned char *dest, size_t *destLen,
		      const unsigned char *source, size_t sourceLen);

/* Bytes of output room that always suffice for one block of block_bytes at `level`, in any frame,
 * a multiple of 16: the slot size (out_stride / out_cap) to give the batch calls, the role of the
 * 1.5 x block the reference allocates (zlibutil_buffer_allocate, applet/7bgzf.c:168).  Levels >= 1
 * code a block longer than HD_SEG_LIMIT in flushed 64 KiB segments (hipdeflate_params.h) and refuse
 * it when the room is below this bound, whatever the data would have needed. */
uint64_t hipdeflate_bound(uint64_t block_bytes, int level);

/* ---- batch API, host buffers ------------------------------------------- */

/* Compress nblocks independent blocks.  Block i is in[in_off[i] .. +in_len[i]).
 * Its output (framed as `frame` says) is written to out + i*out_stride, at most
 * min(out_stride, out_cap) bytes; out_len[i] = bytes written, crc32[i] = CRC-32
 * of the block's INPUT (fcrc32, applet/7bgzf.c:269), status[i] = 0 or 1 (does
 * not fit).  crc32/status may be NULL.  out_stride must be a multiple of 16.
 * Returns 0 if the batch ran (look at status[] per block), else HD_E_*.
 * The room (tests/encode_room.py restates it): min(out_stride, out_cap), at most 65536 in HD_FRAME_BGZF, less the
 * frame's header and trailer, must hold the member --
 *   HD_FRAME_RAW_FLUSH keeps 5 bytes free behind the last data block for the flush suffix, which takes 4 or 5: a
 *     member that would end exactly at the room may be refused;
 *   levels 1..2, a block longer than HD_SEG_LIMIT: the room must cover HD_SEG_WORST whatever the data needs;
 *   HD_FRAME_LATENCY, levels 1..2: a block longer than HD_LAT_SEG_BYTES(level) gets the latency form when the room
 *     covers its worst case (HD_SEGN_WORST), else the ordinary form -- decided per block.  A block longer than
 *     HD_SEG_LIMIT is the exception: it gets the latency form or none, where hip_deflate (and the twin) would fall
 *     back to HD_SEG_BYTES segments in a room between the two worst cases.
 * Stores are whole dwords: where min(out_stride, out_cap) is not a multiple of 4, the rest of its last dword (up to
 * 3 bytes, never past out_stride) may be written too. */
int hipdeflate_batch_deflate(const uint8_t *in, const uint64_t *in_off,
			     const uint32_t *in_len, uint32_t nblocks,
			     int level, int frame,
			     uint8_t *out, uint64_t out_stride, uint32_t out_cap,
			     uint32_t *out_len, uint32_t *crc32, int32_t *status);

/* Decompress nblocks independent raw-DEFLATE streams.  Stream i is
 * in[in_off[i] .. +in_len[i]) (trailing bytes allowed), its output goes to
 * out + out_off[i], capacity out_cap[i]; out_len[i] = bytes produced,
 * crc32[i] = CRC-32 of the OUTPUT (may be NULL), status[i] = 0/1/3 as
 * hip_inflate.  One stream must be shorter than HD_INFLATE_MAX_IN (2^28 bytes, hipdeflate_params.h):
 * the host entry points return HD_E_ARG for a longer one, the _dev entry points (which cannot see
 * in_len) report status 1 / out_len 0 for it. */
int hipdeflate_batch_inflate(const uint8_t *in, const uint64_t *in_off,
			     const uint32_t *in_len, uint32_t nblocks,
			     uint8_t *out, const uint64_t *out_off,
			     const uint32_t *out_cap,
			     uint32_t *out_len, uint32_t *crc32, int32_t *status);

/* hipdeflate_batch_inflate with hip_inflate_flush's stopping rule */
int hipdeflate_batch_inflate_flush(const uint8_t *in, const uint64_t *in_off,
				   const uint32_t *in_len, uint32_t nblocks,
				   uint8_t *out, const uint64_t *out_off,
				   const uint32_t *out_cap,
				   uint32_t *out_len, uint32_t *crc32, int32_t *status);

/* ---- batch API, device-resident buffers --------------------------------- */
/* Same contracts, every pointer is a DEVICE address (hipMalloc'd, or a torch
 * CUDA tensor's data_ptr()); `stream` is a hipStream_t (NULL = default stream).
 * One more rule for hipdeflate_batch_deflate_dev at levels >= 3: the host does not see the lengths, so the parse's
 * records are sized by the slot, and a block longer than min(out_stride, out_cap) is refused (status 1) even where
 * its member would fit.
 * Asynchronous: returns after enqueueing.  `in` and `out` bases must be
 * 16-byte aligned; fastest when every in_off[i] is too (0xff00 and 0x10000 are). */
int hipdeflate_batch_deflate_dev(const void *in, const void *in_off,
				 const void *in_len, uint32_t nblocks,
				 int level, int frame,
				 void *out, uint64_t out_stride, uint32_t out_cap,
				 void *out_len, void *crc32, void *status,
				 void *stream);
int hipdeflate_batch_inflate_dev(const void *in, const void *in_off,
				 const void *in_len, uint32_t nblocks,
				 void *out, const void *out_off, const void *out_cap,
				 void *out_len, void *crc32, void *status,
				 void *stream);

int hipdeflate_batch_inflate_flush_dev(const void *in, const void *in_off,
				       const void *in_len, uint32_t nblocks,
				       void *out, const void *out_off, const void *out_cap,
				       void *out_len, void *crc32, void *status,
				       void *stream);

/* ---- zlib and gzip members, and the size pass ----------------------------------------
 * The decoder's side of HD_FRAME_ZLIB / HD_FRAME_GZIP: nblocks members of RFC 1950 / RFC 1952 (or raw DEFLATE streams,
 * HD_FRAME_RAW) anywhere in a device buffer -- PNG IDATs, the chunks of an array store, HTTP bodies, plain gzip members
 * without a length field -- decoded without the host reading a byte.  Role: libdeflate_deflate_decompress_ex,
 * libdeflate_zlib_decompress_ex (lib/libdeflate/zlib_decompress.c:31-91) and libdeflate_gzip_decompress_ex
 * (gzip_decompress.c:30-133), by frame, per member; and for the size pass the first of the two inflates of
 * applet/7png.c:114-181, which decodes a stream into a throw-away buffer only to learn its size.
 * frame is HD_FRAME_RAW, HD_FRAME_ZLIB or HD_FRAME_GZIP (anything else, HD_FRAME_LATENCY included: HD_E_ARG).  Member i is
 * in[in_off[i] .. +in_len[i]), at any byte offset; bytes behind its trailer are allowed.  All arrays are device arrays
 * (in_off, out_off u64; the others u32, status i32), the calls are asynchronous as hipdeflate_batch_inflate_dev is.
 *
 * hipdeflate_batch_inflate_framed_dev: status[i] is what the reference function answers for member i with out_cap[i]
 * bytes of room -- 0, 1 bad data (header, stream or trailer), 3 does not fit (decided before any check, as there):
 *   gzip   18 bytes at least; 1f 8b 08; a reserved FLG bit (0xe0) is bad data; FEXTRA, FNAME, FCOMMENT and FHCRC must each
 *          leave 8 bytes behind them; FHCRC is skipped, not verified; the CRC-32 and ISIZE (mod 2^32) of the trailer must hold;
 *   zlib   6 bytes at least; FCHECK; CM 8; CINFO <= 7; FDICT is refused; the Adler-32 of the trailer must hold;
 *   the stream may use at most in_len[i] - header - trailer bytes, and the trailer is read at the byte it really ended on.
 * out_len[i] = bytes produced; check[i] (may be NULL) = the CRC-32 (RAW, GZIP) or Adler-32 (ZLIB) of the output;
 * in_used[i] (may be NULL) = header + stream rounded up to a whole byte + trailer, the reference's actual_in_nbytes: added
 * to in_off[i] it is where a member behind this one starts (the walk over concatenated members stays with the caller here;
 * hipdeflate_index_members_any_dev below does it on the device).
 * All three are 0 for a member that fails.  No byte at or behind in_off[i] + in_len[i] is read, whatever a header
 * claims; no byte of out outside [out_off[i], out_off[i] + out_len[i]) is written, beyond what
 * hipdeflate_batch_inflate_dev writes: the decoded prefix of a member that fails, inside its room.  A member of
 * HD_INFLATE_MAX_IN bytes or more has status 1.  out_len and status must not be NULL.
 *
 * hipdeflate_batch_inflate_size_dev writes nothing but its three result arrays (none may be NULL): status[i] is the framed
 * call's with unlimited room, minus the one thing that needs the bytes -- the CRC-32 / Adler-32 value is not examined (the
 * gzip ISIZE is); out_size[i] = the decoded length, in_used[i] as above.  A member that decodes to 2^32 bytes or more has
 * status 3; a member that fails has out_size and in_used 0.  Status 0 therefore means that the framed call with out_cap[i]
 * = out_size[i] can only fail on the check value.  A kernel of its own (one wavefront per member, no window, no output):
 * cheaper than inflating into scratch.
 * Scratch (the payload table, 24 bytes a member) is the library's, grow-only; calls on different streams take turns.
 * nblocks == 0: returns 0 and writes nothing. */
int hipdeflate_batch_inflate_size_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
				      void *out_size /* u32[n] */, void *in_used /* u32[n] */, void *status /* i32[n] */,
				      void *stream);
int hipdeflate_batch_inflate_framed_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
					void *out, const void *out_off, const void *out_cap,
					void *out_len, void *check /* u32[n], may be NULL */, void *in_used /* may be NULL */,
					void *status, void *stream);
/* the host-buffer forms: staged through the device as hipdeflate_batch_inflate is; HD_E_ARG for a member of
 * HD_INFLATE_MAX_IN bytes or more */
int hipdeflate_batch_inflate_size(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				  uint32_t *out_size, uint32_t *in_used, int32_t *status);
int hipdeflate_batch_inflate_framed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				    uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
				    uint32_t *out_len, uint32_t *check, uint32_t *in_used, int32_t *status);

/* Gather the variable-length members produced by batch_deflate_dev into one
 * contiguous stream: member i (out_len[i] bytes at slots + i*stride) goes to
 * dst + dst_off[i], where dst_off is the exclusive prefix sum of out_len (plus
 * this rank's base when the stream is sharded across GPUs -- SURVEY.md 8(e)).
 * dst_off is computed on the device by hipdeflate_scan_sizes_dev: dst_off[i] = base + out_len[0] + ... + out_len[i-1]
 * in 64 bits.  *total (may be NULL) receives the sum of out_len[] alone: it excludes base; nblocks == 0 sets it to 0.
 * hipdeflate_compact_dev wants stride a multiple of 4 and slots 4-byte aligned (else HD_E_ARG), writes member i's
 * out_len[i] bytes and no byte beside them. */
int hipdeflate_scan_sizes_dev(const void *out_len, uint32_t nblocks,
			      uint64_t base, void *dst_off, void *total,
			      void *stream);
int hipdeflate_compact_dev(const void *slots, uint64_t stride,
			   const void *out_len, const void *dst_off,
			   uint32_t nblocks, void *dst, void *stream);
/* The same gather for ONE RANK'S SPAN of a stream sharded across GPUs: dst_off[] holds
 * offsets in the whole concatenated stream (scan_sizes_dev with base = sum of the lower ranks' totals, the
 * one all_gather of the path), `span` is this rank's buffer and span_base the stream offset of its first
 * byte: member i goes to span + (dst_off[i] - span_base).  The rank then pwrite()s the span at span_base --
 * the in-order writer of applet/7bgzf.c:263-272 without moving payload between GPUs. */
int hipdeflate_compact_span_dev(const void *slots, uint64_t stride,
				const void *out_len, const void *dst_off,
				uint32_t nblocks, void *span, uint64_t span_base,
				void *stream);

/* ---- device-resident container decode --------------------------------------------
 * The member table of a stream of gzip members that is already a device buffer (a tensor, the output of
 * hipdeflate_compact_dev, a span handed over by another rank): the four tables hipdeflate_batch_inflate_dev wants plus
 * the CRC-32 of every trailer, made on the device -- the host reads no byte of the blob.  Replaces the serial header walk
 * of the reference's reader, _read_gz_header per member (applet/7bgzf.c:81-131) inside the loop of applet/7bgzf.c:306-328,
 * and gives exactly what that walk gives: it starts at byte 0, takes a member's length from its extra field -- BC (BGZF),
 * MZ (MiGz), IG v1, IG v2 and mgzip, with FNAME / FCOMMENT / FHCRC -- and goes on behind the member until the end.  Bytes
 * inside a member that look like a header do not matter: the chain from byte 0 alone decides.  Member i of the table:
 *   in_off[i]   (u64) offset of its raw DEFLATE payload       in_len[i]   (u32) payload + the 8-byte trailer, as :328 passes it
 *   out_size[i] (u32) ISIZE of its trailer                    out_off[i]  (u64) exclusive prefix sum of out_size
 *   crc_want[i] (u32) CRC-32 of its trailer
 * all five device arrays of max_members entries.  *summary (host memory) says how the walk ended: */
typedef struct hipdeflate_member_summary {
	uint64_t nmembers;    /* members in the table (status 3: members the stream has) */
	uint64_t out_bytes;   /* sum of ISIZE over the table */
	uint64_t end_offset;  /* where the walk stopped; == nbytes when status is 0 */
	uint32_t status;      /* 0 ok | 1 not a member at end_offset | 2 member at end_offset cut off | 3 table too small */
} hipdeflate_member_summary;
/* `blob` must be 16-byte aligned, nbytes is arbitrary (0: no members, status 0); no byte at or behind blob + nbytes is read,
 * whatever the headers claim.  Status 1: the bytes at end_offset rule a member out (magic, FLG, an unknown extra field, a
 * length below header + trailer); status 2: they run out first (inside the header, a name without its NUL, or the member
 * reaches past nbytes).  With status 1 or 2 the table holds the members in front of end_offset, and they are usable.  With
 * status 3 the first max_members members are in the table, nothing is written past them, and end_offset is the end of the
 * last member the stream has.  Entries behind nmembers are never written.  Returns 0 whenever the index ran (the verdict
 * on the data is summary->status), HD_E_* otherwise (HD_E_ARG: blob not aligned, summary NULL).  Scratch -- the candidate
 * list, its successor tables -- is the library's, grow-only; calls on different streams take turns (one call at a time,
 * on the host, for the length of the call).  Work: one streaming read of the blob, O(log candidates) passes over the
 * candidate list, and FNAME / FCOMMENT scans that together read O(nbytes) however many headers the payloads imitate; a
 * single name is scanned by one lane, byte by byte, so a name of megabytes costs what it costs the host walk.
 * (Synchronises the stream.) */
int hipdeflate_index_members_dev(const void *blob, uint64_t nbytes, uint32_t max_members,
				 void *in_off, void *in_len, void *out_size, void *out_off, void *crc_want,
				 hipdeflate_member_summary *summary /* HOST */, void *stream);
/* The trailer check behind the inflate (applet/7bgzf.c:306-328 leaves it to the codec; bgzf_decompress_bytes does it per
 * member on the host): compares what hipdeflate_batch_inflate_dev wrote -- status 0, out_len == out_size, crc32 ==
 * crc_want -- for members 0..nmembers-1, all five device arrays.  *first_bad (host memory) = the index of the first member
 * that disagrees, nmembers if none.  (Synchronises the stream.) */
int hipdeflate_verify_members_dev(const void *status, const void *out_len, const void *crc32,
				  const void *out_size, const void *crc_want, uint32_t nmembers,
				  uint64_t *first_bad /* HOST: index, or nmembers if none */, void *stream);

/* ---- ... and members that state NO length: `cat a.gz b.gz`, the records of a .warc.gz, `gzip >> log.gz` ----------------
 * Role: the loop a serial reader runs over such a file -- inflate one member to learn where it ends, read the trailer, start
 * again behind it (the reader of applet/7gzip.c, called once per member) -- whose every step waits for the one before.
 * hipdeflate_index_members_any_dev makes the same five tables, with the same meaning, as hipdeflate_index_members_dev, for a
 * file whose members may or may not carry a length field; in_off is absolute in blob, out_off starts at 0.  Everything
 * behind it -- hipdeflate_batch_inflate_dev, hipdeflate_verify_members_dev, hipdeflate_read_ranges_dev -- takes the table
 * unchanged.
 *   The walk starts at first_offset (any byte position; first_offset == nbytes: no members, status 0; beyond: HD_E_ARG).  The
 * CANDIDATES are all positions p >= first_offset with 1f 8b 08 and FLG & 0xe0 == 0 whose four bytes lie in front of nbytes.
 * The member at a candidate is read from its window [p, min(nbytes, p + cap)) by one of two rules:
 *   rule A  FEXTRA is set and the extra field is one of the five kinds above, by XLEN and tag: the member is what
 *           hipdeflate_index_members_dev makes of it -- its length is the field's, nothing is decoded, cap is unbounded, and
 *           a field whose length is below header + trailer is BAD (it does not fall through to rule B);
 *   rule B  everything else -- no FEXTRA, or an extra field of any other shape: the header by the rules of
 *           hipdeflate_batch_inflate_framed_dev's HD_FRAME_GZIP (FEXTRA / FNAME / FCOMMENT / FHCRC skipped), the DEFLATE
 *           stream decoded WITHOUT OUTPUT to the end of its final block (a flush point is no stop), the eight trailer bytes
 *           behind the byte the stream ended on, ISIZE equal to the decoded length; cap = max_member_in (0 means
 *           HD_INFLATE_MAX_IN - 1, which is also the most; more: HD_E_ARG).  out_size = the decoded length, crc_want = the
 *           trailer's CRC-32, which is not examined here: hipdeflate_verify_members_dev does that, as for every member.
 *           A member of 2^32 decoded bytes or more is no member (BAD).
 * A candidate is read in stream order -- header fields, stream, trailer -- and the first event decides: a byte that rules a
 * member out is BAD; a needed byte at or behind the window's end is CUT where the window ends at nbytes and TOO LONG where
 * max_member_in ended it.  Only the chain from first_offset decides: a magic inside a stored payload or inside another
 * member is a candidate that nothing links to.  *summary (host memory): */
typedef struct hipdeflate_member_any_summary {
	uint64_t nmembers;     /* members in the table (status 3: members the chain has) */
	uint64_t out_bytes;    /* sum of out_size over the table */
	uint64_t end_offset;   /* where the walk stopped; == nbytes when status is 0 */
	uint64_t ncandidates;  /* positions at or behind first_offset that can start a member */
	uint64_t nsized;       /* of those, the ones that state no known length (rule B) */
	uint32_t status;       /* 0 | 1 not a member at end_offset | 2 member at end_offset cut off | 3 table too small
	                          | 4 the member at end_offset is longer than max_member_in */
} hipdeflate_member_any_summary;
/* status is that of the position the walk stopped at: 1 for BAD and for a position that is no candidate; 2 for CUT, and for
 * fewer than four bytes left whose magic fits as far as it goes; 4 for TOO LONG.  With status 1, 2 or 4 the members in
 * front of end_offset are in the table and usable -- a caller may decode the long member another way (the block index) and
 * resume behind it with first_offset.  Status 3 and the sizing call (max_members == 0, NULL tables) are those of
 * hipdeflate_index_members_dev.  On every blob for which that call answers status 0, this one with first_offset 0 writes
 * the same five tables and the same nmembers, out_bytes and end_offset.
 *   `blob` must be 16-byte aligned; no byte at or behind blob + nbytes is read, nothing behind nmembers entries is written.
 * Stated costs.  Every rule-B candidate is decoded once, one wavefront each, whether the chain reaches it or not: nsized
 * decodes of at most max_member_in bytes.  A true member costs about the size pass of its stream (about half an inflate);
 * a decoy -- chance makes one per 2^27 bytes, a file that embeds .gz files has theirs -- costs one bounded decode, and most
 * end inside their first block header; a blob of adversarial magics costs nsized * max_member_in at the worst, so a caller
 * that does not trust its input passes a bound.  A file of BGZF / MiGz members has nsized == 0 and costs the old call plus
 * one compaction.  Scratch: 48 bytes per candidate, the library's, grow-only.  Returns 0 whenever the index ran.
 * (Synchronises the stream; takes turns as the other indexes do.) */
int hipdeflate_index_members_any_dev(const void *blob, uint64_t nbytes, uint64_t first_offset,
				     uint32_t max_members, uint32_t max_member_in,
				     void *in_off, void *in_len, void *out_size, void *out_off, void *crc_want,
				     hipdeflate_member_any_summary *summary /* HOST */, void *stream);
/* host-buffer form -- the `gzip -dc` of a multi-member file, and the reader of applet/7gzip.c for such files: stages source,
 * runs the index above (twice: the sizing call, then on a table of that size), hipdeflate_batch_inflate_dev and
 * hipdeflate_verify_members_dev.  *destLen: in = room, out = bytes; *in_used (may be NULL) = end_offset.  Returns 0; 1 for
 * index status 1 / 2 / 4 or a member whose inflate or trailer disagrees; 3 when the room is too small, with *destLen = the
 * need; HD_E_*.  A member of HD_INFLATE_MAX_IN bytes or more is status 4 here: such a file is hip_inflate_stream_blocks'. */
int hip_inflate_members(unsigned char *dest, size_t *destLen,
			const unsigned char *source, size_t sourceLen,
			size_t *in_used);

/* Ranged reads on that table -- what a BGZF index is for (`bgzip -b OFFSET -s SIZE`, the chunks of a .bai / .tbi lookup):
 * nqueries ranges [q_begin[q], q_end[q]) of the decoded file are delivered, and only the members they touch are inflated,
 * each once however many queries touch it.  The five tables are those of hipdeflate_index_members_dev for `blob`
 * (nmembers entries); q_begin / q_end are u64 device arrays read according to `kind`: */
#define HD_RANGE_BYTES   0   /* q_begin/q_end: offsets in the decoded file, [begin, end) */
#define HD_RANGE_VOFFSET 1   /* q_begin/q_end: virtual offsets, HIPDEFLATE_VOFFSET(coffset, uoffset), [begin, end) */
/* With total = out_off[nmembers-1] + out_size[nmembers-1] (taken on the device):
 *   HD_RANGE_BYTES    begin > end is refused (q_status 1); end is clipped to total; begin >= total gives length 0, status 0.
 *   HD_RANGE_VOFFSET  v names the decoded position U(v) = out_off[m] + uoffset, where m is the member that STARTS at
 *                     coffset = v >> 16 (member 0 starts at 0, member i at in_off[i-1] + in_len[i-1]: in_len counts the
 *                     trailer, so this holds for all five member kinds) and uoffset = v & 0xffff <= out_size[m]; coffset ==
 *                     the end of the last member with uoffset 0 names total.  Everything else is refused (q_status 1): a
 *                     coffset inside a member, the offset of a payload, a uoffset past ISIZE, U(begin) > U(end).
 * A query of 2^32 bytes or more after clipping is refused with q_status 2 (q_len is 32 bits wide: split the range).  A
 * refused query has q_len 0, takes no room in dst and does not disturb the others; the call still returns 0.
 * Output: q_len[q] (u32) bytes of query q at dst + dst_off[q], dst_off (u64) the exclusive prefix sum of q_len made on the
 * device, q_status[q] (i32); all three device arrays of nqueries entries.  No byte of dst outside [0, out_bytes) is
 * written; dst needs no alignment.  Overlapping, nested, duplicate and unsorted queries each get their own copy.
 * A member is inflated if and only if an accepted query takes at least one byte of it: members of ISIZE 0 (the EOF
 * block) and queries of length 0 select nothing.  *summary (host memory): */
typedef struct hipdeflate_range_summary {
	uint64_t out_bytes;   /* sum of q_len[] */
	uint64_t nselected;   /* distinct members decoded */
	uint64_t sel_bytes;   /* sum of their ISIZE */
	uint64_t nrefused;    /* queries with q_status != 0 */
	uint64_t bad_member;  /* status 2: lowest index, in the CALLER's table, of a decoded member whose inflate
	                       * disagrees with its trailer; nmembers otherwise */
	uint32_t status;      /* 0 ok | 2 a decoded member is bad | 3 dst too small (| 1 the table is refused:
	                       * hipdeflate_stream_read_ranges_dev alone) */
} hipdeflate_range_summary;
/* Status 3 (out_bytes > dst_cap): nothing is inflated and dst is not touched; q_len, dst_off, q_status and the summary are
 * complete, so a call with dst == NULL and dst_cap == 0 is the sizing call.  Status 2: a selected member disagrees with its
 * trailer by the rules of hipdeflate_verify_members_dev; dst is written all the same, the bytes of the queries that touch
 * a bad member are unspecified, and bad_member names the lowest one.  nmembers == 0 or nqueries == 0: returns 0 with a
 * zero summary (bad_member == nmembers) and writes nothing.  Returns 0 whenever the read ran (the verdict is
 * summary->status), HD_E_ARG for a NULL summary, a kind that is neither of the two, a blob that is not 16-byte aligned, a NULL table or query array where
 * there are entries, or dst == NULL with dst_cap != 0, and HD_E_NOMEM if the scratch cannot grow.  The decoded members
 * live in scratch of the library (sel_bytes of it, grow-only); calls take turns with one another and with the index.
 * (Synchronises the stream: nselected, sel_bytes and out_bytes size the inflate launch and the scratch.) */
int hipdeflate_read_ranges_dev(const void *blob,
			       const void *in_off, const void *in_len, const void *out_size, const void *out_off,
			       const void *crc_want, uint32_t nmembers,
			       int kind, const void *q_begin, const void *q_end, uint32_t nqueries,
			       void *dst, uint64_t dst_cap,
			       void *dst_off /* u64[nqueries] */, void *q_len /* u32[nqueries] */, void *q_status /* i32[nqueries] */,
			       hipdeflate_range_summary *summary /* HOST */, void *stream);

/* ---- one stream from a device buffer, coded in parallel chunks ----------------------
 * Role of the single-stream writers of the reference: zlibstdio / zlibrawstdio (zlibrawstdio_compress.h:260-307), the IDAT
 * of applet/7png.c:296-331, a .gz any tool reads with one inflate().  There one stream is one serial deflate ("one stream =
 * no block parallelism"); here the buffer is cut into chunks of chunk_bytes, every chunk is coded as a block of its own by
 * the batch kernels, and the stream is
 *     header | chunk 0 .. chunk n-1 | 03 00 | trailer
 *   header   none (HD_FRAME_RAW) | 78 da (HD_FRAME_ZLIB) | the ten bytes HD_FRAME_GZIP writes: 1f 8b 08 00 <mtime = 0> 02 00
 *   chunk i  in exactly the bytes hipdeflate_batch_deflate_dev(..., HD_FRAME_RAW_FLUSH) gives block i: such chunks concatenate
 *   trailer  none | Adler-32 big-endian | CRC-32, then nbytes mod 2^32, little-endian
 * The CRC-32 / Adler-32 of the whole input is folded on the device from the chunks' own (zlib's crc32_combine /
 * adler32_combine, all chunks at once).  Chunks are independent -- no window across a seam, pigz -i's trade; at levels 1..2 a
 * chunk longer than HD_SEG_LIMIT is segmented inside as any block is.  nbytes == 0: no chunks, check 0 (CRC-32) / 1 (Adler-32).
 * frame is HD_FRAME_RAW, HD_FRAME_ZLIB or HD_FRAME_GZIP (anything else, HD_FRAME_LATENCY included: HD_E_ARG); chunk_bytes a
 * multiple of 16 in [16, 64 MiB]; in, dst and strm 16-byte aligned (else HD_E_ARG).  *summary (host memory): */
typedef struct hipdeflate_stream_summary {
	uint64_t out_bytes;   /* encode: bytes of the whole stream (status 3: bytes it needs); decode: bytes written to out */
	uint64_t in_bytes;    /* encode: nbytes; decode: bytes of stream consumed (trailer included) */
	uint64_t bad_chunk;   /* status 1/2: lowest chunk at fault; nchunks if it is the whole-stream check, header or terminator */
	uint32_t nchunks;
	uint32_t check;       /* CRC-32 (RAW, GZIP) or Adler-32 (ZLIB) of the whole uncompressed data */
	uint32_t status;      /* 0 ok | 1 not such a stream / bad table | 2 a chunk or the check disagrees | 3 room too small */
} hipdeflate_stream_summary;
/* Bytes of dst that always suffice (0 for a chunk_bytes that is refused). */
uint64_t hipdeflate_stream_bound(uint64_t nbytes, uint32_t chunk_bytes, int level, int frame);
/* The encoder.  chunk_off (device, u64[nchunks + 1], may be NULL): chunk_off[i] = the stream offset of chunk i,
 * chunk_off[nchunks] = the offset of the 03 00 -- the table the decoder below wants, a dictzip RA table for a plain stream.
 * Scratch is the library's: the slots, hipdeflate_bound(chunk_bytes, level) each, of one WINDOW of chunks -- at most
 * HD_STREAM_WINDOW_BYTES (hipdeflate_params.h) of them, so the scratch does not grow with the input; the stream offset and
 * the check run on from window to window.  Room: dst_cap below the need gives status 3 with out_bytes = the need -- every
 * window is still coded to learn it, so dst == NULL with dst_cap == 0 is the sizing call -- and no byte at or behind dst +
 * dst_cap is written (what is in front of it is unspecified then); hipdeflate_stream_bound always suffices.  Status 2 (a
 * chunk the batch encoder refused; bad_chunk names the lowest) does not happen with slots of the bound.  Returns 0 whenever
 * the call ran (the verdict is summary->status), HD_E_* otherwise.  Calls take turns with one another, with
 * hipdeflate_read_ranges_dev and with the index.  hipdeflate_stall_count() stays 0.  (Synchronises the stream, once a window.) */
int hipdeflate_stream_deflate_dev(const void *in, uint64_t nbytes, uint32_t chunk_bytes, int level, int frame,
				  void *dst, uint64_t dst_cap, void *chunk_off /* u64[nchunks + 1], may be NULL */,
				  hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* The same encoder with every chunk PRIMED by the input in front of it -- what pigz writes by default, where the call above is
 * pigz -i.  Arguments, refusals, statuses, summary, chunk_off, the sizing call, the windows of HD_STREAM_WINDOW_BYTES and the
 * turn-taking are hipdeflate_stream_deflate_dev's, rule for rule, and so is the layout: header | chunk 0 .. n-1 | 03 00 |
 * trailer, every chunk ending in 00 00 ff ff on a byte boundary at chunk_off[i + 1] - 4.  hipdeflate_stream_bound covers this form
 * too (a chunk's worst case is still stored + flush).  The one difference, at levels 3..9: chunk i, which starts at input byte
 * s = i * chunk_bytes, is parsed with
 *     prime(i) = min(32768, s) & ~1023
 * bytes in front of it in the table and the window.  No token is made for those bytes and the chunk's CRC-32 / Adler-32 covers
 * the chunk alone, but its matches may name any of them: distances go up to 32768 across the seam.  The rounding down to 1024
 * keeps the chunk's first byte on a piece boundary of the parse (no match crosses one: hipdeflate_params.h HD_WG_CUT) and
 * in + s - prime(i) 16-byte aligned; with chunk_bytes a multiple of 1024 every chunk behind the first 32 KiB has the whole
 * window.  A chunk's tokens are those of a one-block parse of (its history || itself) behind the seam.  Chunk 0 has no history: a
 * stream of one chunk is byte for byte hipdeflate_stream_deflate_dev's, and so is chunk 0 of any stream.
 * Levels 0..2 have windows of 4 KiB or none, and a fresh window per 0xff00 bytes costs them under 1 % as it is: there the call
 * writes exactly the bytes of hipdeflate_stream_deflate_dev.
 * What the form costs a READER: every zlib, and any serial inflate, reads it as it reads any stream.  But the decode by chunk
 * table, hipdeflate_stream_inflate_dev, answers status 2 at the first chunk that reaches back (never wrong bytes): its chunks
 * are no longer independent.  The decode for this form is the carry pair below (hipdeflate_stream_index_carry_dev /
 * hipdeflate_stream_inflate_carry_dev), which takes 8..11 times the time of the full-flush decode (README).  This form is for
 * streams that serial inflaters will read -- a .gz, a zlib buffer, a PNG IDAT: it has the one-block ratio at any chunk size --;
 * the independent form stays the default for everything this library decodes itself. */
int hipdeflate_stream_deflate_carry_dev(const void *in, uint64_t nbytes, uint32_t chunk_bytes, int level, int frame,
					void *dst, uint64_t dst_cap, void *chunk_off /* u64[nchunks + 1], may be NULL */,
					hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* ---- preset dictionary: thousands of small blocks against one shared history --------
 * A small block with an empty window compresses badly; zlib's remedy is the preset dictionary.  Roles: deflateSetDictionary
 * (lib/zlib/deflate.c:550-614) in front of every block's deflate, inflateSetDictionary (lib/zlib/inflate.c:1298-1329) in front
 * of every member's inflate, and for HD_FRAME_ZLIB the FDICT bit and the DICTID field of the header (written at
 * lib/zlib/deflate.c:1010, read at lib/zlib/inflate.c:810-822) -- for all blocks of a launch at once, with one dictionary.
 * `dict` is a device pointer of any alignment (the library stages what it uses into aligned scratch of its own, once per call);
 * dict == NULL with dict_len != 0 is HD_E_ARG.  Calls take turns on that scratch as they do on the token slabs.
 *
 * hipdeflate_batch_deflate_dict_dev: hipdeflate_batch_deflate_dev's arguments and contract -- refusals, statuses, rooms, the
 * refusal of a block longer than its slot at levels >= 3 -- without the frame: the output is HD_FRAME_RAW, every member ends in a
 * final block, and there is no latency form.  At levels 3..9 block b is parsed with the LAST
 *     used = min(32768, dict_len) & ~1023
 * bytes of the dictionary as its history: no token is made for them, crc32[b] covers the block alone, and the block's matches
 * may name any of them -- distances go up to 32768 into the dictionary.  The rounding down to 1024 keeps the seam on a piece
 * boundary of the parse (hipdeflate_params.h HD_WG_CUT), exactly as prime(i) above does: a block's tokens are those of a one-block
 * parse of (that history || block) behind the seam.  Two limits follow and are meant: a dictionary SHORTER THAN 1024 BYTES is
 * accepted and NOT USED, and UP TO 1023 BYTES AT THE FRONT of a dictionary below 32 KiB + 1023 are not used (give a
 * dictionary whose length is a multiple of 1024, its most useful bytes last, as for zlib).  A reader sets the dictionary it was
 * given, whole: inflateSetDictionary keeps its last 32 KiB, which contain the used bytes.
 * dict_len == 0, used == 0 and levels 0..2 (windows of 4 KiB or none) write exactly the bytes of hipdeflate_batch_deflate_dev(...,
 * HD_FRAME_RAW, ...), as hipdeflate_stream_deflate_carry_dev does at those levels.  A zlib (RFC 1950) wrapper with FDICT on the
 * encode side is not built: the caller who wants one writes 2 + 4 header bytes and the Adler-32 around the raw member.
 * The history's hash table is the same for every block of the call: it is built once (one workgroup) and every block whose
 * (history || block) fits the parse's 64 KiB ring copies it instead of replaying up to 32 pieces; longer blocks replay.  The
 * bytes are the same either way.  The emit kernel follows the parse (not beside it).  hipdeflate_stall_count() stays 0.
 *
 * hipdeflate_batch_inflate_dict_dev: hipdeflate_batch_inflate_framed_dev's arguments, arrays, result semantics (out_len, check,
 * in_used, status), read and write bounds and its refusal of members of HD_INFLATE_MAX_IN bytes, with frame HD_FRAME_RAW or
 * HD_FRAME_ZLIB (anything else: HD_E_ARG).  Every member starts with a full window: only the last D = min(32768, dict_len) bytes
 * of the dictionary can be named (no rounding here), and a distance d at output position p is valid iff d <= p + D -- otherwise
 * status 1, as without a dictionary.  check[i] and the zlib trailer cover the output alone.
 *   HD_FRAME_ZLIB: the rules above, except that FDICT is allowed.  With FDICT four more header bytes hold DICTID, big-endian,
 *     which must equal the Adler-32 of the WHOLE dictionary as given, all dict_len bytes (taken on the device) -- otherwise status
 *     1; so is a member cut inside DICTID, and FDICT with dict_len == 0 (zlib's Z_NEED_DICT).  in_used counts the six header
 *     bytes.  A member WITHOUT FDICT is decoded without the dictionary, as zlib does.
 *   HD_FRAME_RAW: every member is decoded with the dictionary.
 * With dict_len == 0, RAW and FDICT-free members get the verdicts, lengths and bytes of hipdeflate_batch_inflate_framed_dev,
 * which is unchanged and keeps refusing FDICT.  (A room within 32 KiB of 2^32 bytes counts as that much shorter.) */
int hipdeflate_batch_deflate_dict_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int level,
				      const void *dict, uint32_t dict_len,
				      void *out, uint64_t out_stride, uint32_t out_cap,
				      void *out_len, void *crc32, void *status, void *stream);
int hipdeflate_batch_inflate_dict_dev(const void *in, const void *in_off, const void *in_len, uint32_t nblocks, int frame,
				      const void *dict, uint32_t dict_len,
				      void *out, const void *out_off, const void *out_cap,
				      void *out_len, void *check /* u32[n], may be NULL */, void *in_used /* may be NULL */,
				      void *status, void *stream);
/* host-buffer forms: hipdeflate_batch_deflate's and hipdeflate_batch_inflate_framed's arguments and staging, the dictionary a
 * host buffer too; the same bytes and answers as the device calls' */
int hipdeflate_batch_deflate_dict(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks,
				  int level, const uint8_t *dict, uint32_t dict_len, uint8_t *out, uint64_t out_stride,
				  uint32_t out_cap, uint32_t *out_len, uint32_t *crc32, int32_t *status);
int hipdeflate_batch_inflate_dict(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint32_t nblocks, int frame,
				  const uint8_t *dict, uint32_t dict_len, uint8_t *out, const uint64_t *out_off,
				  const uint32_t *out_cap, uint32_t *out_len, uint32_t *check, uint32_t *in_used, int32_t *status);
/* test entry: on != 0 makes every block of a dictionary encode replay the history (no table snapshot); 0 restores the default */
void hipdeflate_test_dict_replay(int on);

/* The inverse -- the device-resident form of what a dictzip reader does with its RA table (applet/7dictzip.c:318-323): given
 * the table, the chunks are inflated side by side, chunk i by the flush-rule batch inflate into out + i * chunk_bytes with
 * exactly its size as room, and the result is held to the trailer.  Streams of other writers qualify if they are cut the
 * same way (zlib: Z_FULL_FLUSH behind every chunk_bytes of input, then Z_FINISH with no input left).
 *   status 1  out_bytes is not what nchunks and chunk_bytes allow (nchunks = ceil(out_bytes / chunk_bytes)); nbytes is too
 *             short for header, 03 00 and trailer; chunk_off does not ascend strictly inside [header, nbytes - 2 - trailer];
 *             a chunk of HD_INFLATE_MAX_IN bytes or more; chunk_off[nchunks] is not nbytes - 2 - trailer or the bytes there
 *             are not 03 00; the header is not one (ZLIB: CM 8, window <= 32 KiB, no dictionary, FCHECK; GZIP: 1f 8b 08 and
 *             FLG 0).  bad_chunk = the lowest entry of chunk_off at fault, nchunks for its last entry, the header and the
 *             lengths.  Nothing is inflated.
 *   status 3  out_cap < out_bytes.  Nothing is inflated.  (Status 1 comes first.)
 *   status 2  bad_chunk = i: chunk i's inflate status is non-zero or its length is wrong (check is unspecified then);
 *             bad_chunk = nchunks: every chunk is fine but the folded check, or the gzip ISIZE, disagrees with the trailer.
 *             HD_FRAME_RAW has no trailer to disagree with.
 * With status 0 and 2 out_bytes and in_bytes are the arguments', with 1 and 3 they are 0.  The kernels bound every read by
 * nbytes whatever the table says.  chunk_off holds nchunks + 1 entries.  Returns 0 whenever the call ran.  (Synchronises the
 * stream; takes turns as the encoder does.) */
int hipdeflate_stream_inflate_dev(const void *strm, uint64_t nbytes, int frame,
				  const void *chunk_off, uint32_t nchunks, uint32_t chunk_bytes, uint64_t out_bytes,
				  void *out, uint64_t out_cap, hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* ---- ... and the same decode for a stream whose table nobody kept ----------------------
 * A .gz, zlib or raw stream written in flush form -- by the encoder above, by zlib with Z_FULL_FLUSH, by pigz -i, a dictzip
 * file without its RA field -- carries its own table: every chunk ends in an empty stored block, whose last four bytes are
 * 00 00 ff ff on a byte boundary.  hipdeflate_stream_index_dev finds it, by the method of the member index: one streaming
 * read of the payload region [header, nbytes - trailer) lists every position with those four bytes in front of it, plus
 * the first payload byte (candidate 0); one wavefront per candidate decodes, writing no byte, from there to whichever
 * comes first -- a FLUSH POINT, the end of a non-final stored block with LEN == 0, or the end of a FINAL block -- over at
 * most min(max_chunk_in, what is left of the payload region) bytes; a piece that ends in a flush point names the candidate
 * behind it, and the chain from candidate 0 alone decides.  Markers inside a chunk -- in a stored payload, or by chance --
 * cost a decode and change nothing.  A chunk whose matches reach back over its own start (a sync flush, which keeps the
 * window) does not decode from that start: the chain stops there with status 1 and is never decoded wrong.  A stream
 * without flush points is one row.  Row i of the table:
 *   in_off[i]   (u64) where the piece starts          in_len[i]   (u32) its exact length, marker included
 *   out_size[i] (u32) bytes it decodes to             out_off[i]  (u64) exclusive prefix sum of out_size
 * all four device arrays of max_chunks entries.  The final piece is a row of its own: for a stream of the encoder above rows
 * 0..n-1 are the chunks, row n is the 03 00 with size 0, and in_off[0..n] equals its chunk_off[0..n] -- where the encoder codes
 * every chunk whole.  At levels 1..2 it codes a chunk longer than HD_SEG_LIMIT as full-flush segments; every segment is a row
 * then, and chunk_off is a subsequence of in_off.  Rows of size 0 (two flushes in a row) stay in the table.  *summary (host
 * memory): */
typedef struct hipdeflate_stream_index_summary {
	uint64_t nchunks;      /* rows in the table (status 3: rows the stream has) */
	uint64_t out_bytes;    /* sum of out_size over the table */
	uint64_t end_offset;   /* status 0: first byte behind the trailer; else where the chain stopped */
	uint64_t ncandidates;
	uint32_t hdr_bytes;
	uint32_t status;       /* 0 ok | 1 the piece at end_offset does not decode (bad data, reaches back over its start, longer than
	                          max_chunk_in, 2^32 bytes of output) or the header is refused | 2 the stream is cut: no final block
	                          before the bytes run out, or no room for the trailer | 3 table too small */
} hipdeflate_stream_index_summary;
/* frame is HD_FRAME_RAW (no header), HD_FRAME_ZLIB or HD_FRAME_GZIP; the header is held to the rules of
 * hipdeflate_batch_inflate_framed_dev (gzip: FEXTRA / FNAME / FCOMMENT / FHCRC allowed, so files of gzip and pigz qualify), on
 * the first HD_INFLATE_MAX_IN - 1 bytes of the stream at the most.  strm must be 16-byte aligned; no byte at or behind strm +
 * nbytes is read.  A marker that would put a candidate at or behind nbytes - trailer does not count.  max_chunk_in bounds
 * one piece's input; 0 means HD_INFLATE_MAX_IN - 1, which is also the most (more: HD_E_ARG).
 *   status 0  the chain's last row ended in a final block, and the trailer's bytes lie behind it.  Bytes behind the trailer
 *             are allowed and are not looked at: end_offset says where a following member would start, and the walk over
 *             concatenated members is the caller's (or hipdeflate_index_members_any_dev's).  The trailer's contents are not examined (the decode below does that).
 *   status 1  the piece that starts at end_offset does not decode: bad data, a distance past the bytes the piece has put out,
 *             2^32 bytes of output, or more than max_chunk_in bytes of input with payload left behind them; or the header is
 *             refused (end_offset 0, hdr_bytes 0, ncandidates 0).
 *   status 2  the piece that starts at end_offset needed a bit at or behind nbytes - trailer, or a flush point is the last
 *             payload byte (end_offset = nbytes - trailer then); or nbytes is below the frame's header and trailer (18 / 6
 *             bytes, end_offset 0, ncandidates 0).  A stream cut short anywhere, trailer included, ends like this unless the
 *             cut leaves an element the rules refuse.
 *   status 3  more rows than max_chunks: the first max_chunks rows are in the table, nothing is written past them, nchunks is
 *             the number the stream has, out_bytes the sum over the table, and end_offset and the verdict that status 3
 *             replaces are those of the whole chain -- max_chunks == 0 with NULL tables is the sizing call.
 * With status 1 or 2 the rows in front of end_offset are in the table and usable with hipdeflate_batch_inflate_flush_dev.
 * Returns 0 whenever the index ran (the verdict is summary->status), HD_E_* otherwise.  Scratch -- the bitmap, the candidate
 * list, five words a candidate -- is the library's, grow-only; calls take turns with the member index and the other stream
 * calls.  Work: one streaming read, one piece decode per candidate, O(log candidates) passes over the list.  An honest
 * writer leaves about one marker by chance per 2^32 compressed bytes, and more only where stored payloads hold the four
 * bytes; a stream made to hurt -- stored payloads full of markers -- buys one decode of at most max_chunk_in bytes per
 * candidate, of which most end within a block header, and never a wrong table.  (Synchronises the stream.) */
int hipdeflate_stream_index_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_chunks, uint32_t max_chunk_in,
				void *in_off /* u64 */, void *in_len /* u32 */, void *out_size /* u32 */, void *out_off /* u64 */,
				hipdeflate_stream_index_summary *summary /* HOST */, void *stream);
/* The decode on such a table: hipdeflate_stream_inflate_dev behind its table check, for rows of uneven size.  Row i goes by
 * the flush-rule batch inflate into out + out_off[i] with exactly out_size[i] as room, the rows' checks are folded, and the
 * result is held to the trailer, which is read behind the last row (in_off[n-1] + in_len[n-1]), wherever nbytes is.  The
 * four tables are device arrays of nchunks entries, in the index's layout.  Status and fields are hipdeflate_stream_summary's:
 *   status 1  nchunks is 0 (a stream has its final row); the header is refused or nbytes too short for header and trailer;
 *             a row starts in front of the header, ends behind nbytes - trailer, overlaps its successor or comes after it, or
 *             has HD_INFLATE_MAX_IN bytes or more; out_off is not the exclusive prefix sum of out_size.  bad_chunk = the
 *             lowest row at fault, nchunks for the header and the lengths.  Nothing is inflated.
 *   status 3  out_cap < out_off[n-1] + out_size[n-1]; out_bytes is that need.  Nothing is inflated.  (Status 1 comes first.)
 *   status 2  bad_chunk = i: row i's inflate status is non-zero or its length is not out_size[i] (check is unspecified then);
 *             bad_chunk = nchunks: every row is fine but the folded check, or the gzip ISIZE, disagrees with the trailer.
 * With status 0 and 2 out_bytes is the rows' total and in_bytes the offset behind the trailer.  No read and no write depends
 * on what the table claims beyond what the check has held it to.  strm 16-byte aligned, out of any alignment.  Returns 0
 * whenever the call ran.  (Synchronises the stream; takes turns as the index does.) */
int hipdeflate_stream_inflate_table_dev(const void *strm, uint64_t nbytes, int frame,
					const void *in_off, const void *in_len, const void *out_size, const void *out_off,
					uint32_t nchunks, void *out, uint64_t out_cap,
					hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* host-buffer form: stage, index, decode; the table stays on the device and the scratch grows with the stream.  *destLen in =
 * room, out = bytes.  0; 1 = not such a stream (index status 1 or 2) or it disagrees with its trailer; 3 = the room is too
 * small, *destLen = the need.  *in_used (may be NULL) = the index's end_offset: with 0 and 3 the first byte behind the trailer. */
int hip_inflate_stream(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame,
		       size_t *in_used);
/* ---- ... and a stream whose flushes CARRY the window: pigz, zlib's Z_SYNC_FLUSH ----------------------
 * The writers people have -- pigz in its default mode, every zlib writer that calls deflate(Z_SYNC_FLUSH), a dictzip-like
 * writer that did not reset the window -- end a chunk in the same empty stored block, but the next chunk's matches reach
 * into the 32 KiB in front of it.  The index above stops at the first such chunk (status 1).  The two calls below decode
 * such a stream side by side all the same, by the two-pass marker method of pugz / rapidgzip.
 *
 * hipdeflate_stream_index_carry_dev is hipdeflate_stream_index_dev -- the same method, candidates, summary, max_chunk_in and
 * header rules -- with one more table, reach (u32[max_chunks]): reach[i] = the furthest a match of row i goes back over the
 * row's first byte, 0 for a row that stands alone, 32768 at the most.  A distance past the bytes a piece has put out is no
 * longer a reason not to decode it (no distance is bad by itself: 32768 is DEFLATE's most); instead, behind the chain and
 * the prefix sum, the first row of the table with reach[i] > out_off[i] -- it reaches back over the start of the stream --
 * ends the chain: status 1, end_offset = in_off[i], nchunks = i, out_bytes = out_off[i], and the rows in front stay
 * usable.  A stream whose first token reaches back is status 1 with nchunks 0, as before.  With more rows than max_chunks
 * the reach rule is applied to the rows in the table only: a row there that breaks it gives the verdict just stated, and
 * otherwise the answer is status 3 with nchunks = the chain's length, as above -- a second call with a table of that size
 * gives the final verdict.  On every stream for which hipdeflate_stream_index_dev answers status 0 this call answers the
 * same summary and the same four tables, with reach all 0. */
int hipdeflate_stream_index_carry_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_chunks, uint32_t max_chunk_in,
				      void *in_off /* u64 */, void *in_len /* u32 */, void *out_size /* u32 */, void *out_off /* u64 */,
				      void *reach /* u32 */, hipdeflate_stream_index_summary *summary /* HOST */, void *stream);
/* The decode on such a table: hipdeflate_stream_inflate_table_dev with the reach column, the same summary and statuses, in
 * this order:
 *   status 1  everything hipdeflate_stream_inflate_table_dev answers status 1 for; or reach[i] > 32768 or reach[i] >
 *             out_off[i].  bad_chunk = the lowest row at fault by either rule.  Nothing is decoded.
 *   status 3  out_cap < out_off[n-1] + out_size[n-1]; out_bytes is that need.  Nothing is decoded.
 *   status 2  bad_chunk = i: row i does not decode by the flush rule, is not out_size[i] long, or reaches further back than
 *             reach[i] says; bad_chunk = nchunks: every row is fine but the folded check, or the gzip ISIZE, disagrees with
 *             the trailer.
 * The table is a hint that is checked, never trusted: a row writes at most out_size[i] bytes at out_off[i], and names a
 * byte in front of itself only within reach[i], which the check has held to the bytes the stream has there.  The rows are
 * taken in GROUPS, in stream order: the consecutive rows whose out_off lies in the same multiple of HD_CARRY_GROUP_BYTES
 * (hipdeflate_params.h; a row is never split), the largest reach of a group taken on the device, one small record per
 * group read by the host.  A group in which no row reaches back goes through the flush-rule batch inflate into place
 * exactly as hipdeflate_stream_inflate_table_dev does it -- a plain single-member .gz and every full-flush stream take
 * only this path, and it needs no scratch.  Any other group takes three launches, none of which waits for another
 * workgroup: every row decoded by one wavefront into 16-bit SYMBOLS (a byte, or "the byte this far in front of my start");
 * one workgroup that walks the rows in order with the running 32 KiB window in LDS and makes every row's last 32 KiB
 * final; all rows side by side turning the rest of their symbols into bytes.  The CRC-32 (RAW, GZIP) / Adler-32 (ZLIB) of
 * such a group is taken from its bytes in pieces of HD_CARRY_CHECK_PIECE behind the third launch, and folded; the check
 * runs on from group to group.  Scratch: 2 bytes per output byte of the largest group that takes the marker path, the
 * library's, grow-only; HD_E_NOMEM if it cannot grow.  With status 2 the bytes of out are unspecified, and groups behind
 * the bad row's may not have been decoded.  strm 16-byte aligned, out of any alignment.  Returns 0 whenever the call ran.
 * (Synchronises the stream, once a group; takes turns as the index does.) */
int hipdeflate_stream_inflate_carry_dev(const void *strm, uint64_t nbytes, int frame,
					const void *in_off, const void *in_len, const void *out_size, const void *out_off,
					const void *reach, uint32_t nchunks, void *out, uint64_t out_cap,
					hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* host-buffer form: hip_inflate_stream with the carry index and the carry decode; the same arguments and return values */
int hip_inflate_stream_carry(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame,
			     size_t *in_used);
/* test entry: the group size of hipdeflate_stream_inflate_carry_dev in bytes (0 restores HD_CARRY_GROUP_BYTES), so that a
 * stream of a few hundred KiB walks several groups; the decoded bytes do not depend on it */
void hipdeflate_test_carry_group(uint64_t bytes);
/* test entry: ms4[0..3] = the milliseconds the marker path's passes -- decode, tails, resolve, check and fold -- took since
 * the last call, by events around their launches (one more wait per group while it is on); the call turns the timing on,
 * NULL turns it off */
void hipdeflate_test_carry_times(double *ms4);
/* ---- ... and a PLAIN stream, which has no flush point at all: gzip, zlib.compress, a PNG's IDAT ----------------------
 * Role: the reader of applet/7gzip.c:8-116 and of zlibrawstdio, one serial inflate there.  Most .gz files, zlib buffers and
 * IDATs hold one stream that nobody flushed; for such a stream both indexes above answer "one row", and one wavefront decodes
 * the file.  What such a stream does have is BLOCKS, which start at any BIT.  The two calls below are the carry index and
 * the carry decode for rows that start and end on a bit.
 *
 * hipdeflate_stream_index_blocks_dev follows the method of hipdeflate_stream_index_dev with a header rule in the place of the
 * 00 00 ff ff marker.  Candidate 0 is the first payload bit, 8 * hdr_bytes, whatever stands there.  Every other candidate
 * is a bit position p behind it at which a NON-FINAL DYNAMIC block header could start: the bits read BFINAL 0, BTYPE 2, HLIT
 * (5 bits), HDIST (5), HCLEN (4), then HCLEN + 4 precode lengths of 3 bits, all 17 + 3 (HCLEN + 4) of them in front of
 * nbytes - trailer, and the precode is one the decoder takes: with K = the sum of 2^(7 - len) over the non-zero lengths,
 * K == 128, K == 0, or one non-zero length that is 1.  Nothing else is examined, so the rule drops no header the decoder
 * would take; random bits pass it at 5.13e-4 of the positions, one candidate per 244 bytes of stream.  One wavefront per
 * candidate then decodes from that bit, block after block, without output (a PIECE): to the end of a final block, or to
 * the end of a non-final block with BFINAL 0 / BTYPE 2 in the three bits behind it.  So a piece never runs through a
 * non-final dynamic header except its own first one; static and stored blocks, and the final block, ride with the piece
 * in front of them, and a flush point is no stop.  A piece that ends in front of such a header links to the candidate at
 * that bit, and only the chain from candidate 0 decides: bits in a stored payload or inside a token that look like a header
 * are candidates that nothing links to.  max_chunk_in bounds one piece's input in bytes (0: HD_INFLATE_MAX_IN - 1, also the
 * most) -- a false candidate costs one bounded decode, and most end inside their header.
 *   Behind the chain its pieces are MERGED, on the device: a row is the run of consecutive pieces whose out_off lies in the
 * same multiple of row_bytes (0: HD_BLOCK_ROW_BYTES; a piece is never split, so row_bytes 1 gives a row per piece), and its
 * reach is the largest of reach_j - (out_off_j - out_off_row) over its pieces, 0 at the least.  The table, device arrays of
 * max_rows entries: in_off (u64) = the BIT offset of the row's first block header in the stream; in_len (u32) = its length
 * in BITS, below 2^31; out_size, out_off, reach as the carry index has them.  The rows tile the payload bit for bit.
 *   status 0  the chain's last piece ended in a final block and the trailer's bytes lie behind it: end_offset = the first
 *             byte behind the trailer, end_bit = the bit behind the final block.  The trailer's contents are not examined.
 *   status 1  the piece at end_bit does not decode, or the header rule refuses the bits there although they are all present,
 *             or the stream's own header is refused (all fields 0); or, as in the carry index, the first row of the table
 *             with reach[i] > out_off[i], or with more than max_chunk_in bytes of stream (a run of empty blocks makes such
 *             a row; so does a long span without a dynamic header, which is one piece), ends the chain: nrows = i,
 *             out_bytes = out_off[i], end_bit = in_off[i], and the rows in front stay usable.
 *   status 2  the piece at end_bit needed a bit at or behind nbytes - trailer, or the header there does not fit in front of
 *             it, or there is no payload.
 *   status 3  the chain has more rows than max_rows: nrows = that number, the table holds the first max_rows, out_bytes is
 *             their sum; the two row rules are applied to the rows in the table only, as in the carry index.  max_rows == 0
 *             with NULL tables is the sizing call.
 * In every status but 0, end_offset = end_bit / 8.  npieces = the pieces of the whole chain, ncandidates = the list's length.
 * Stated limits.  Only non-final dynamic headers are found: a stream of static or stored blocks only (this library's level 1,
 * incompressible data) is one piece and one row, decoded by one wavefront, and status 1 where it is longer than
 * max_chunk_in.  Scratch, the library's, grow-only: 40 bytes per candidate -- at one per 244 bytes of stream, 4.4 M
 * candidates and 180 MB for 1 GiB -- one bit per 16 stream bytes, and 40 bytes per piece of the chain.
 * strm 16-byte aligned; no byte at or behind strm + nbytes is read.  Returns 0 whenever the call ran.  (Synchronises the
 * stream; takes turns as the other indexes do.) */
typedef struct hipdeflate_block_index_summary {
	uint64_t nrows;        /* rows in the table (status 3: rows the chain has) */
	uint64_t npieces;      /* pieces of the chain, before the merge */
	uint64_t out_bytes;    /* sum of out_size over the table */
	uint64_t end_offset;   /* bytes.  status 0: the first byte behind the trailer; else end_bit / 8 */
	uint64_t end_bit;      /* the exact bit where the chain stopped */
	uint64_t ncandidates;
	uint32_t hdr_bytes;
	uint32_t status;
} hipdeflate_block_index_summary;
int hipdeflate_stream_index_blocks_dev(const void *strm, uint64_t nbytes, int frame, uint32_t max_rows, uint32_t max_chunk_in,
				       uint32_t row_bytes, void *in_off /* u64, bits */, void *in_len /* u32, bits */,
				       void *out_size /* u32 */, void *out_off /* u64 */, void *reach /* u32 */,
				       hipdeflate_block_index_summary *summary /* HOST */, void *stream);
/* The decode on such a table: hipdeflate_stream_inflate_carry_dev for bit rows, with the same summary and the same order of
 * statuses.  The table is checked, never trusted:
 *   status 1  nrows is 0, or the header is refused; a row starts in front of bit 8 * hdr_bytes, ends behind bit
 *             8 * (nbytes - trailer), overlaps its successor or comes after it, or has in_len >= 2^31; out_off is not the
 *             exclusive prefix sum of out_size; reach[i] > 32768 or reach[i] > out_off[i].  bad_chunk = the lowest row at
 *             fault.  Nothing is decoded.
 *   status 3  out_cap < out_off[n-1] + out_size[n-1]; out_bytes is that need.  Nothing is decoded.
 *   status 2  bad_chunk = i: row i, decoded from bit in_off[i] & 7 of byte in_off[i] / 8, does not end behind a final block or
 *             behind a block that ends on bit in_len[i] exactly (a block end past in_len[i] is this), is not out_size[i]
 *             long, or reaches further back than reach[i]; bad_chunk = nrows: the folded check, or the gzip ISIZE, disagrees
 *             with the trailer, which is read at the byte behind the last row's last bit.
 * A row writes at most out_size[i] bytes at out_off[i].  The groups of the carry decode run as they stand, but there is no
 * fast path -- the flush-rule batch inflate starts on a byte -- so every group takes the marker path: scratch 2 bytes per
 * output byte of the largest group.  hipdeflate_test_carry_group sizes the groups here too. */
int hipdeflate_stream_inflate_blocks_dev(const void *strm, uint64_t nbytes, int frame,
					 const void *in_off, const void *in_len, const void *out_size, const void *out_off,
					 const void *reach, uint32_t nrows, void *out, uint64_t out_cap,
					 hipdeflate_stream_summary *summary /* HOST */, void *stream);
/* host-buffer form: hip_inflate_stream with the block index and the block decode; the same arguments and return values.  The
 * index runs with max_chunk_in = HD_BLOCK_PIECE_IN (hipdeflate_params.h) first and with 0 only where that answers status 1, so
 * a stream whose pieces are longer than that, or that is bad, is indexed twice. */
int hip_inflate_stream_blocks(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen, int frame,
			      size_t *in_used);
/* test entry: the header rule alone.  pos[] (u64, device) holds n bit positions of the stream strm[0, nbytes), whose bits at
 * and behind 8 * nbytes do not exist; verdict[] (u32, device) gets 0 = the rule refuses the position, 1 = it accepts it,
 * 2 = the header does not fit in front of the end.  (Does not synchronise.) */
int hipdeflate_test_block_headers_dev(const void *strm, uint64_t nbytes, const void *pos, uint32_t n, void *verdict, void *stream);
/* test entry: ms4[0..3] = the milliseconds the block index's passes -- candidates, pieces, chain, merge -- took since the
 * last call, by events around their launches; the call turns the timing on, NULL turns it off */
void hipdeflate_test_blocks_times(double *ms4);
/* test entry: out2[0] = the candidates of the last index call made while that timing was on whose piece got past its own first
 * block header, out2[1] = those whose piece decodes to its stop */
void hipdeflate_test_blocks_counts(uint64_t *out2);
/* test entry: the candidate list alone, by the two passes the index uses.  strm[0, nbytes) 16-byte aligned; the list is `first`
 * (a bit position below 8 * nbytes, whatever stands there) and every position behind it that the header rule accepts,
 * ascending; *count HOST = its length, pos[] (u64, device) gets the first min(*count, max_pos).  (Synchronises the stream.) */
int hipdeflate_test_block_candidates_dev(const void *strm, uint64_t nbytes, uint64_t first, void *pos, uint32_t max_pos,
					 uint64_t *count /* HOST */, void *stream);
/* ---- ... and a SEEK INDEX on either table: the window in front of every row, and ranged reads on it ----------------------
 * Role: the index with windows of zran, gztool and rapidgzip.  The two decodes above decode the whole stream every time; data
 * that is resident in HBM is read more than once, and to get one byte of it that is a full decode.  A row of the carry table
 * or the block table names bytes in front of itself only within reach[i], and the row decoders turn every such reference
 * into a marker that points straight into those reach[i] bytes.  Keep the reach[i] bytes in front of every row once, behind
 * one full decode, and every row stands alone: a ranged read decodes only the rows it touches, in no order, and a read of
 * the whole stream runs no serial pass at all.
 *   What the windows cost: reach[i] <= 32768, so the windows hold at most 32 KiB a ROW, whatever the row's size -- row_bytes
 * of the block index (the chunk size of a flushing writer) is the knob.  At the default 128 KiB rows they are at most a
 * quarter of the decoded size; at 4,096-byte rows of word-shaped text they were seven times the data.
 *
 * hipdeflate_stream_windows_dev makes the windows.  out[0, out_bytes) is the decoded stream: what
 * hipdeflate_stream_inflate_carry_dev or hipdeflate_stream_inflate_blocks_dev wrote with status 0 for this table.  Only the
 * output-side columns are used -- out_size, out_off, reach, device arrays of nrows entries -- so the call serves byte rows and
 * bit rows alike.  win_off: u64[nrows + 1], win: win_cap bytes, row_check: u32[nrows] (may be NULL: no checks are taken), all
 * device memory.  *summary (host memory): */
typedef struct hipdeflate_window_summary {
	uint64_t win_bytes;   /* win_off[nrows] = sum of reach; with status 3: the need */
	uint64_t bad_row;     /* status 1: the lowest row at fault; nrows otherwise */
	uint32_t status;      /* 0 ok | 1 the table is refused | 3 win_cap too small */
} hipdeflate_window_summary;
/*   status 1  out_off is not the exclusive prefix sum of out_size from 0, or the total is not out_bytes; reach[i] > 32768 or
 *             reach[i] > out_off[i].  bad_row = the lowest row at fault; nrows == 0 (a stream has its final row) names row 0.
 *             Nothing is written.
 *   otherwise win_off is the exclusive prefix sum of reach with nrows + 1 entries, always written: win == NULL with
 *             win_cap == 0 is the sizing call.
 *   status 3  win_cap < win_off[nrows].  Neither win nor row_check is touched.
 *   status 0  win[win_off[i] .. win_off[i+1]) = out[out_off[i] - reach[i] .. out_off[i]); row_check[i] = the CRC-32 of row i's
 *             out_size[i] bytes, whatever the frame (a row of size 0: 0).  No byte of win at or behind win_cap is written.
 * out and win need no alignment.  Returns 0 whenever the call ran.  (Synchronises the stream; takes turns as the indexes do.) */
int hipdeflate_stream_windows_dev(const void *out, uint64_t out_bytes,
				  const void *out_size, const void *out_off, const void *reach, uint32_t nrows,
				  void *win_off /* u64[nrows + 1] */, void *win, uint64_t win_cap,
				  void *row_check /* u32[nrows] */, hipdeflate_window_summary *summary /* HOST */, void *stream);
/* The ranged read: hipdeflate_read_ranges_dev for one stream.  unit says what in_off / in_len count: */
#define HD_ROWS_BYTES 0   /* bytes: the table of hipdeflate_stream_index_carry_dev */
#define HD_ROWS_BITS  1   /* bits:  the table of hipdeflate_stream_index_blocks_dev */
/* The five columns are the index's, win_off / win / row_check what hipdeflate_stream_windows_dev made of them (win_bytes =
 * the bytes of win that may be read; row_check may be NULL: the rows' bytes are not checked then).  The queries are
 * HD_RANGE_BYTES queries of hipdeflate_read_ranges_dev, rule for rule: begin > end is refused (q_status 1), end is clipped to
 * the total, begin at or behind the total gives length 0, 2^32 bytes or more after clipping give q_status 2; duplicate,
 * nested and unsorted queries each get a copy of their own; a refused query disturbs nothing.  dst_off, q_len, q_status and
 * the summary behave as in that call; bad_member names a ROW.  A row is decoded if and only if an accepted query takes at
 * least one byte of it.  In this order:
 *   HD_E_ARG  a NULL summary; a unit that is neither of the two; a frame other than RAW / ZLIB / GZIP; strm not 16-byte
 *             aligned; NULL tables where there are rows; NULL query arrays where there are queries; dst == NULL with dst_cap != 0.
 *   status 1  (a value this call alone gives the struct) the table breaks a rule of its unit's decode call -- everything
 *             hipdeflate_stream_inflate_carry_dev / hipdeflate_stream_inflate_blocks_dev answers status 1 for on the rows, the
 *             reach rule included -- or the stream's header is refused (bad_member = nrows); or win_off[0] != 0, or
 *             win_off[i+1] - win_off[i] != reach[i], or row i's window ends behind win_bytes (so a table that is right but for
 *             win_off[nrows] > win_bytes names the first row whose window does).  bad_member = the lowest row at fault.
 *             Nothing is decoded, and the query arrays are not written.
 *   status 3  the sum of q_len exceeds dst_cap.  Nothing is decoded; the three query arrays and the summary are complete --
 *             dst == NULL with dst_cap == 0 is the sizing call.
 *   status 2  bad_member = the lowest selected row, by the caller's table, that fails: it does not decode by its unit's rule
 *             (the flush rule; the exact end bit), is not out_size[i] long, reaches further back than reach[i], or -- with
 *             row_check -- the CRC-32 of its bytes is not row_check[i].  dst is unspecified for the queries that touch a
 *             failed row; every other query has its bytes.
 * The stream's trailer is NOT examined: the full decode in front of the windows call did that, and a read sees only the
 * rows it touches.  Without row_check a wrong byte in win goes unnoticed.  nrows == 0 or nqueries == 0 returns 0 with a zero
 * summary (bad_member = nrows).  No byte of strm at or behind nbytes, none of win at or behind win_bytes is read; no byte of
 * dst outside [0, out_bytes) is written; what the table states is checked, never trusted.
 *   The passes: the table check; the queries resolved as the member call does it; the selected rows' tables compacted; the
 * selected rows decoded to 16-bit symbols in groups of HD_CARRY_GROUP_BYTES of SELECTED output (hipdeflate_test_carry_group
 * sizes them here too) by the row decoder of the unit, as it stands; all rows of the group side by side turning every
 * symbol into its byte or win[win_off[i] + reach[i] - distance], eight symbols to a load and eight bytes to a store; the
 * checks; the gather of hipdeflate_read_ranges_dev.  Scratch, the library's, grow-only: 2 bytes per output byte of the
 * largest group, and sel_bytes, the sum of the selected rows' out_size -- so a read of the whole stream holds the stream
 * twice beside dst: this limit is stated, not lifted.  Returns 0 whenever the call ran.  (Synchronises the stream, once a
 * group; takes turns with the indexes and the other stream calls.)  There is no host-buffer form. */
int hipdeflate_stream_read_ranges_dev(const void *strm, uint64_t nbytes, int frame, int unit,
				      const void *in_off, const void *in_len, const void *out_size, const void *out_off, const void *reach,
				      const void *win_off, const void *win, uint64_t win_bytes, const void *row_check /* may be NULL */, uint32_t nrows,
				      const void *q_begin, const void *q_end, uint32_t nqueries,
				      void *dst, uint64_t dst_cap, void *dst_off, void *q_len, void *q_status,
				      hipdeflate_range_summary *summary /* HOST */, void *stream);
/* the fold on its own: check[] / len[] device arrays of n parts (u32 each, n < 2^31), kind 0 = CRC-32, 1 = Adler-32; *result HOST.
 * The check of the concatenation of the parts from the parts' own: the role of crc_append (the hosts' serial fold, after
 * zlib's crc32_combine) with one lane per part -- part i contributes check[i] moved over the S_i bytes behind it, S_i a
 * 64-bit suffix sum, so the parts may total anything below 2^64.  A part of length 0 is an identity whatever its check says;
 * n == 0 gives 0 / 1.  (Synchronises the stream.) */
int hipdeflate_check_combine_dev(const void *check, const void *len, uint32_t n, int kind, uint32_t *result, void *stream);
/* host-buffer form of the encoder: stages through the device; *destLen in = room, out = bytes; 0, or 1 = does not fit */
int hip_deflate_stream(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen,
		       int level, int frame, uint32_t chunk_bytes);
/* ... and of hipdeflate_stream_deflate_carry_dev: the same bytes as the device call's */
int hip_deflate_stream_carry(unsigned char *dest, size_t *destLen, const unsigned char *source, size_t sourceLen,
			     int level, int frame, uint32_t chunk_bytes);
/* test entry: chunks per window of the encoder (0 restores the default) */
void hipdeflate_test_stream_window(uint32_t chunks);

/* ---- streaming encoder: the host pipeline either side of the kernels ------------
 * Role of the read / compress / write loop of applet/7bgzf.c:159-293 (7migz.c:130-244)
 * for a stream of fixed-size blocks (the last may be short).  `depth` batches are in
 * flight: the caller fills PINNED input memory directly (no staging copy), H2D copy,
 * kernels and D2H copy of different batches overlap on their own streams, and a
 * result is ONE contiguous run of finished members in block order (the device
 * gathers them), so writing it out is a single write().  Calls on one pipe may come
 * from two threads: one doing input()/submit(), one doing result().
 *
 *   p   = hipdeflate_pipe_open(level, HD_FRAME_BGZF, 0xff00, 4096, 3);
 *   buf = hipdeflate_pipe_input(p, &cap);  n = read(0, buf, cap);  hipdeflate_pipe_submit(p, n);
 *   hipdeflate_pipe_result(p, &data, &nbytes, &nblocks);  write(1, data, nbytes);
 */
typedef struct hipdeflate_pipe hipdeflate_pipe;
/* block_bytes must be a multiple of 16 (0xff00, 0x10000 and b * 1024 are); 2 <= depth <= 16; NULL otherwise.
 * A slot is free again only when its result has been fetched AND a later call of hipdeflate_pipe_result has released
 * it: a single thread may call hipdeflate_pipe_input only while (batches submitted and not yet fetched) + (1 if it
 * holds a result) < depth, otherwise that call waits for ever.  hipdeflate_unpipe has the same limits and the same rule. */
hipdeflate_pipe *hipdeflate_pipe_open(int level, int frame, uint32_t block_bytes,
				      uint32_t blocks_per_batch, int depth);
/* pinned buffer for the next batch, *cap = block_bytes * blocks_per_batch; waits for
 * a free slot (one whose result has been fetched and released); NULL on error */
uint8_t *hipdeflate_pipe_input(hipdeflate_pipe *p, size_t *cap);
/* enqueue the batch just filled (nbytes <= cap, 0 allowed); returns at once */
int hipdeflate_pipe_submit(hipdeflate_pipe *p, size_t nbytes);
/* the oldest submitted batch: waits for it.  *data stays valid until the next call of
 * hipdeflate_pipe_result on this pipe (also one that answers HD_E_ARG).  Returns 0; 1 if a block did not fit its slot
 * (hipdeflate_bound(block_bytes, level), at most 65536 in HD_FRAME_BGZF: cannot happen for BGZF/MiGz block sizes,
 * does for incompressible blocks of 65536 bytes in HD_FRAME_BGZF) -- such a block has out_len 0 in the member table
 * and adds no bytes to the run, the other members are in place; HD_E_*; HD_E_ARG when nothing is pending */
int hipdeflate_pipe_result(hipdeflate_pipe *p, const uint8_t **data, size_t *nbytes,
			   uint32_t *nblocks);
/* The members of the result last fetched (valid as long as its data): their sizes, their offsets inside the run --
 * the device's size prefix scan, i.e. the compressed offsets a block index needs (bgzip's .gzi, BAM virtual
 * offsets; the role of the index member of applet/7gzinga.c:173-193) -- and the CRC-32 of each block's input.
 * Any of the three may be NULL.  After a batch of 0 bytes there is no table: all three come back NULL.  HD_E_ARG when
 * no result is held. */
int hipdeflate_pipe_members(hipdeflate_pipe *p, const uint32_t **out_len, const uint64_t **dst_off,
			    const uint32_t **crc32);
/* BAM / tabix virtual file offset of byte `uoffset` of the block whose member starts at `coffset` */
#define HIPDEFLATE_VOFFSET(coffset, uoffset) (((uint64_t)(coffset) << 16) | (uint64_t)((uoffset) & 0xffff))
void hipdeflate_pipe_close(hipdeflate_pipe *p);
/* the same pipe on entry `index` of the device list: one pipe per device and batches dealt round robin is how
 * hd7bgzf -g N drives N cards from one in-order reader and one in-order writer */
hipdeflate_pipe *hipdeflate_pipe_open_on(int index, int level, int frame, uint32_t block_bytes,
					 uint32_t blocks_per_batch, int depth);

/* ---- streaming decoder: the same pipeline in the other direction -----------------
 * Role of the read / inflate / write loop of applet/7bgzf.c:295-365.  The caller reads
 * compressed bytes into pinned memory, pre-scans the member headers there (the serial
 * BSIZE walk of _read_gz_header, applet/7bgzf.c:81-131) and submits the table; a
 * result is the batch's output as ONE contiguous run (member i at the exclusive
 * prefix sum of out_size[]).  Threading as for hipdeflate_pipe. */
typedef struct hipdeflate_unpipe hipdeflate_unpipe;
hipdeflate_unpipe *hipdeflate_unpipe_open(uint32_t max_members, size_t in_cap, size_t out_cap, int depth);
uint8_t *hipdeflate_unpipe_input(hipdeflate_unpipe *p, size_t *cap);
/* member i: raw DEFLATE at in_off[i] .. +in_len[i] of the buffer (trailing bytes allowed),
 * inflating to exactly out_size[i] bytes (the ISIZE of its trailer); sum(out_size) <= out_cap.
 * HD_E_ARG, with the batch still the caller's to submit again, for nmembers > max_members, sum(out_size) > out_cap,
 * a member reaching past in_cap, or a member of HD_INFLATE_MAX_IN bytes or more */
int hipdeflate_unpipe_submit(hipdeflate_unpipe *p, const uint64_t *in_off, const uint32_t *in_len,
			     const uint32_t *out_size, uint32_t nmembers);
/* oldest submitted batch; returns 0, or the first member's non-zero inflate status
 * (1 bad data / 3 does not fit, also used when a member is shorter than out_size), or HD_E_* */
int hipdeflate_unpipe_result(hipdeflate_unpipe *p, const uint8_t **data, size_t *nbytes);
void hipdeflate_unpipe_close(hipdeflate_unpipe *p);
hipdeflate_unpipe *hipdeflate_unpipe_open_on(int index, uint32_t max_members, size_t in_cap, size_t out_cap, int depth);

/* ---- latency contexts: small synchronous batches ----------------------------------
 * For callers that hold a FEW blocks and wait for them: the LD_PRELOAD hook (htslib's worker threads hand over
 * one 0xff00-byte block each), the per-block codecs, a thread-per-block loop like applet/7bgzf.c:159-277 ported
 * as it stands.  A context owns pinned device-visible buffers and a stream: the caller writes block i straight
 * into hipdeflate_lat_input(c, i), hipdeflate_lat_run() codes n blocks (frame | HD_FRAME_LATENCY: several
 * wavefronts per block) and returns when the members are in hipdeflate_lat_output(c, i, ...).  No staging copy,
 * no copy-engine transfer: the kernels read and write the pinned memory themselves.  One thread at a time per
 * context; different contexts run concurrently. */
typedef struct hipdeflate_lat hipdeflate_lat;
hipdeflate_lat *hipdeflate_lat_open(int level, int frame, uint32_t max_blocks, uint32_t max_block_bytes);
/* where block i's input goes (max_block_bytes of pinned memory, 16-byte aligned); NULL if i is out of range */
uint8_t *hipdeflate_lat_input(hipdeflate_lat *c, uint32_t i);
/* code blocks 0..n-1 of in_len[i] bytes; synchronous; 0 if the batch ran (per-block status via _output) */
int hipdeflate_lat_run(hipdeflate_lat *c, const uint32_t *in_len, uint32_t n);
/* member i of the last run: its bytes (pinned, valid until the next run), size, CRC-32 of the input, status */
const uint8_t *hipdeflate_lat_output(hipdeflate_lat *c, uint32_t i, uint32_t *out_len, uint32_t *crc32, int32_t *status);
void hipdeflate_lat_close(hipdeflate_lat *c);
hipdeflate_lat *hipdeflate_lat_open_on(int index, int level, int frame, uint32_t max_blocks, uint32_t max_block_bytes);

/* scratch bytes batch_deflate_dev needs per launch for `level` (0 for level <= 1): the token slabs of the
 * fused kernel plus, for blocks up to 256 KiB (max_block = the slot stride), the tokens and histograms of one
 * sub-batch of the parse + emit kernel pair -- at most 8.25 GiB however large the batch.  The library keeps
 * its own grow-only scratch; this is informational. */
uint64_t hipdeflate_scratch_bytes(uint32_t nblocks, uint32_t max_block, int level);

/* ---- LD_PRELOAD hook ----------------------------------------------------- */
/* Same signature and return values as bgzf_compress.c:39: 0 ok; -1 if *dlen < 26 (28 for the EOF block) or the
 * device is missing; 1 on codec error.  slen == 0 yields the canned 28-byte EOF block.  BGZF_METHOD (parsed once,
 * bgzf_compress.c:53-113: name + trailing digits = level): `hip<level>` is this library's coder (`hip` alone =
 * level 1); UNSET means level 6, as the reference's unset means its zlib at 6 (bgzf_compress.c:54,:102); a name of
 * the reference's table (zlib, libdeflate, igzip, ...) or an unknown one is served by the hip coder at the level
 * the reference would have used for it, with one line on stderr -- a BGZF_METHOD=libdeflate6 left in the
 * environment keeps writing.  There is no CPU codec behind any name.  Calls from concurrent htslib worker threads
 * are micro-batched into latency-mode launches on pinned memory: a batch closes when every caller inside the hook
 * has joined, when nobody has joined for HIPDEFLATE_LINGER_US (8), or after HIPDEFLATE_BATCH_US (60); at most
 * HIPDEFLATE_INFLIGHT (2) batches are on a device at once; batch contexts are spread over the device list.  With up to
 * HIPDEFLATE_MERGE_CALLERS (16) callers a batch that is merely complete waits for the batch on the device (HIPDEFLATE_MERGE_INFLIGHT, 1)
 * and then up to HIPDEFLATE_REJOIN_US (30) for that batch's callers, so that a handful of callers share ONE launch instead of
 * taking turns in two.  Every level has one form behind this call (HD_FRAME_LATENCY above). */
int bgzf_compress(void *dst, size_t *dlen, const void *src, size_t slen, int level);

/* device self-test of the wave primitives (scan, CRC folding); 0 = pass */
int hipdeflate_selftest(void);
/* test entry: the code lengths the device's Huffman construction gives nvec frequency vectors of nsyms
 * (2..288) symbols each under a length limit of maxbits (1..15); lens_out[nvec * nsyms] */
int hipdeflate_test_build_lengths(const uint32_t *freq, uint32_t nvec, uint32_t nsyms, uint32_t maxbits,
				  uint8_t *lens_out);
/* test entry: the schedule of the workgroup levels' throughput form (levels >= 3, launches of 512 blocks and more) --
 * keep = the emit wavefronts a CU keeps resident beside the parse (0..3; 0: none stay, the launches that follow the parses do all
 * the emit work), sub_cap = a cap on the blocks of a sub-batch (0 = none: 17 GiB of records), so that a launch of a few thousand blocks
 * walks the path of a 16 GiB one (two record buffers, the gates between sub-batches).  The bytes do not depend on either.  Process-wide;
 * (3, 0) restores the defaults. */
void hipdeflate_test_beside(int keep, uint32_t sub_cap);
/* test entry: the grid (wavefronts) of the last gather kernel that hipdeflate_compact_dev / hipdeflate_compact_span_dev launched
 * on the calling thread's device context; 0 before the first.  A gather launched while an encode of hipdeflate_batch_deflate_dev
 * (level >= 1, enough blocks to fill the device) is still queued or running in ANOTHER stream, into other slots than the
 * gather's, runs on a small grid: it has that kernel's time to spare and takes less from it.
 * HIPDEFLATE_GATHER_GRID=full|beside|auto (default auto; read at every launch) forces either grid.  The bytes do not depend on it. */
uint32_t hipdeflate_test_compact_grid(void);

#ifdef __cplusplus
}
#endif
#endif
