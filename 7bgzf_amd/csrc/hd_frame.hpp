// hd_frame.hpp -- RFC 1950 / RFC 1952 members around the batch inflate: the decoder's side of HD_FRAME_ZLIB / HD_FRAME_GZIP.
//
// Role: libdeflate_zlib_decompress_ex (lib/libdeflate/zlib_decompress.c:31-91) and libdeflate_gzip_decompress_ex
// (gzip_decompress.c:30-133) for thousands of members at once, each anywhere in a device buffer:
//   k_frame_open    member (in_off, in_len) -> payload offset, payload length, header verdict, by those functions' rules;
//   k_inflate_framed / k_inflate_size (hd_inflate.hpp, hd_inflate_size.hpp) on that payload table;
//   k_frame_close   the trailer at the byte the stream really ended on, against the CRC-32 the inflate folded or the
//                   Adler-32 k_chunk_adler made of the output, and the final status, out_len, check and in_used.
// HD_FRAME_RAW has neither step: the caller's tables are the payload table.
#pragma once
#include "hd_device.hpp"
#include "../../include/hipdeflate.h"

namespace hd {

// where the zero-terminated field that starts at src[pos] ends: the position behind its NUL, n where src[pos, n) holds
// none (gzip_decompress.c:80-93 reads on to the end of the input and no further).  64 bytes a step: a name of kilobytes
// is not one lane's byte loop.
__device__ __forceinline__ uint32_t frame_skip_cstring(const uint8_t *src, uint32_t pos, uint32_t n, uint32_t lane)
{
	for (uint32_t base = pos; base < n; base += 64) {
		const uint32_t i = base + lane;
		const uint32_t c = i < n ? (uint32_t)src[i] : 1u;
		const uint64_t z = __ballot(c == 0);
		if (z)
			return base + (uint32_t)__ffsll((unsigned long long)z);
	}
	return n;
}

// One wavefront per member; every lane walks the same header (the loads are one address), the names are scanned by all.
// No byte at or behind in_off + in_len is read.  A member the rules refuse has payload length 0 at its own start.
__global__ __launch_bounds__(64) void k_frame_open(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
						    const uint32_t *__restrict__ in_len, uint32_t nmembers, int frame,
						    uint64_t *__restrict__ p_off, uint32_t *__restrict__ p_len, int32_t *__restrict__ verdict)
{
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	if (b >= nmembers)
		return;
	const uint64_t off = in_off[b];
	const uint8_t *src = in + off;
	const uint32_t n = in_len[b];
	uint32_t pos = 0, foot = 0;
	bool ok = n < HD_INFLATE_MAX_IN;          // (the payload is shorter still; the host entry points answer HD_E_ARG first)
	if (frame == HD_FRAME_ZLIB) {
		// zlib_decompress.c:45-66: six bytes at least, FCHECK, CM 8, CINFO <= 7, no FDICT
		foot = 4;
		ok = ok && n >= 6;
		if (ok) {
			const uint32_t hdr = ((uint32_t)src[0] << 8) | src[1];
			ok = hdr % 31 == 0 && ((hdr >> 8) & 15) == 8 && (hdr >> 12) <= 7 && !((hdr >> 5) & 1);
			pos = 2;
		}
	} else {
		// gzip_decompress.c:45-100: eighteen bytes at least, 1f 8b 08, no reserved FLG bit; every optional field must
		// leave the trailer's eight bytes behind it; FHCRC is skipped, not verified
		foot = 8;
		ok = ok && n >= 18;
		if (ok) {
			const uint32_t flg = src[3];
			ok = src[0] == 0x1f && src[1] == 0x8b && src[2] == 8 && !(flg & 0xe0);
			pos = 10;
			if (ok && (flg & 4)) {                                     // FEXTRA
				const uint32_t xlen = src[10] | ((uint32_t)src[11] << 8);
				pos = 12;
				ok = n - pos >= xlen + 8;
				pos += xlen;
			}
			if (ok && (flg & 8)) {                                     // FNAME
				pos = frame_skip_cstring(src, pos, n, lane);
				ok = n - pos >= 8;
			}
			if (ok && (flg & 16)) {                                    // FCOMMENT
				pos = frame_skip_cstring(src, pos, n, lane);
				ok = n - pos >= 8;
			}
			if (ok && (flg & 2)) {                                     // FHCRC
				pos += 2;
				ok = n - pos >= 8;
			}
		}
	}
	if (lane == 0) {
		p_off[b] = ok ? off + pos : off;
		p_len[b] = ok ? n - foot - pos : 0u;
		verdict[b] = ok ? HD_OK : HD_BAD_DATA;
	}
}

// k_frame_open for HD_FRAME_ZLIB members that may name a PRESET DICTIONARY (hipdeflate_batch_inflate_dict_dev): the same rules,
// but FDICT is allowed -- four more header bytes, DICTID big-endian, which must be *dict_adler, the Adler-32 of the call's whole
// dictionary (with_dict == 0: none was given and FDICT is refused).  plain[b] = 1 for a member without FDICT: it is decoded
// without the dictionary, as zlib's inflate does.  One lane's work per member, 256 members a workgroup.
__global__ __launch_bounds__(256) void k_dict_open(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
						    const uint32_t *__restrict__ in_len, uint32_t nmembers, const uint32_t *__restrict__ dict_adler,
						    uint32_t with_dict, uint64_t *__restrict__ p_off, uint32_t *__restrict__ p_len,
						    int32_t *__restrict__ verdict, uint32_t *__restrict__ plain)
{
	const uint32_t b = blockIdx.x * 256 + threadIdx.x;
	if (b >= nmembers)
		return;
	const uint64_t off = in_off[b];
	const uint8_t *src = in + off;
	const uint32_t n = in_len[b];
	uint32_t pos = 0, fdict = 0;
	bool ok = n < HD_INFLATE_MAX_IN && n >= 6;
	if (ok) {
		const uint32_t hdr = ((uint32_t)src[0] << 8) | src[1];
		ok = hdr % 31 == 0 && ((hdr >> 8) & 15) == 8 && (hdr >> 12) <= 7;
		fdict = (hdr >> 5) & 1;
		pos = 2;
	}
	if (ok && fdict) {
		ok = with_dict && n >= 10;                               // DICTID, and the trailer's four bytes behind it
		if (ok) {
			const uint32_t id = ((uint32_t)src[2] << 24) | ((uint32_t)src[3] << 16) | ((uint32_t)src[4] << 8) | src[5];
			ok = id == *dict_adler;
			pos = 6;
		}
	}
	p_off[b] = ok ? off + pos : off;
	p_len[b] = ok ? n - 4 - pos : 0u;
	verdict[b] = ok ? HD_OK : HD_BAD_DATA;
	plain[b] = fdict ? 0u : 1u;
}

// One lane per member, behind k_inflate_framed (and k_chunk_adler for HD_FRAME_ZLIB): status[] and out_len[] hold the
// inflate's answer and get the member's.  A member whose header was refused or whose inflate failed keeps that status;
// HD_INSUFFICIENT_SPACE was decided before any check, as in the reference.  A member that fails has out_len, check and
// in_used 0.  used[i] <= the payload's length, so the trailer lies inside the member.
__global__ __launch_bounds__(256) void k_frame_close(const uint8_t *__restrict__ in, const uint64_t *__restrict__ in_off,
						      const uint64_t *__restrict__ p_off, const int32_t *__restrict__ verdict,
						      const uint32_t *__restrict__ used, const uint32_t *__restrict__ chk, uint32_t nmembers,
						      int frame, uint32_t *out_len, uint32_t *check, uint32_t *in_used, int32_t *status)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= nmembers)
		return;
	int32_t st = verdict[i] ? HD_BAD_DATA : status[i];
	uint32_t len = out_len[i], c = chk[i], u = 0;
	if (st == HD_OK) {
		const uint8_t *t = in + p_off[i] + used[i];
		if (frame == HD_FRAME_ZLIB) {
			if (((((uint32_t)t[0] << 24) | ((uint32_t)t[1] << 16) | ((uint32_t)t[2] << 8) | t[3])) != c)
				st = HD_BAD_DATA;
			u = 4;
		} else {
			const uint32_t crc = t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
			const uint32_t isize = t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
			if (crc != c || isize != len)
				st = HD_BAD_DATA;
			u = 8;
		}
		u += (uint32_t)(p_off[i] - in_off[i]) + used[i];
	}
	if (st != HD_OK)
		len = c = u = 0;
	out_len[i] = len;
	status[i] = st;
	if (check)
		check[i] = c;
	if (in_used)
		in_used[i] = u;
}

} // namespace hd
