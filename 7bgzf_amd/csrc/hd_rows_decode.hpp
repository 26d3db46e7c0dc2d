// hd_rows_decode.hpp -- the text of the row decoder of the marker path, one kernel per inclusion (no include guard).
//
// The includer defines HD_ROWS_DECODE_KERNEL (the kernel's name), HD_ROWS_DECODE_ARGS (its argument struct, CarryDecodeArgs
// or a struct derived from it) and HD_ROWS_DECODE_BITS:
//   false  k_carry_decode (hd_carry.hpp, which describes the kernel): in_off and in_len in bytes, the row ends by the flush rule;
//   true   k_blocks_decode (hd_blocks.hpp): in_off and in_len in BITS; the row starts at bit in_off & 7 of byte in_off >> 3 and
//          ends behind a final block, or behind a block that ends on bit in_len exactly; a block end past in_len fails the row.
// Everything that differs stands under `if constexpr (BITS)` or folds on it.
__global__ __launch_bounds__(64) void HD_ROWS_DECODE_KERNEL(HD_ROWS_DECODE_ARGS a)
{
	constexpr bool BITS = HD_ROWS_DECODE_BITS;
	__shared__ CarryLds L;
	const uint32_t lane = threadIdx.x;
	if (blockIdx.x >= a.nrows)
		return;
	const uint32_t row = a.r0 + blockIdx.x;
	// (BITS: the bit the row starts on in its byte, and the bit it ends on, from that byte)
	[[maybe_unused]] const uint32_t sh = BITS ? (uint32_t)a.in_off[row] & 7 : 0u, end_bits = BITS ? sh + a.in_len[row] : 0u;
	const uint32_t n = BITS ? (end_bits + 7) >> 3 : a.in_len[row];      // < HD_INFLATE_MAX_IN: k_stream_check_rows (BITS: in_len < 2^31, so <= 2^28 + 1, one byte
	                                                                    // or two over what InfReader's callers keep to: its 32-bit bit counts, 8 n + 64 + 24 at the most, still fit)
	const uint8_t *src = a.in + (BITS ? a.in_off[row] >> 3 : a.in_off[row]);
	const uint32_t cap = a.out_size[row], claim = a.reach[row];
	uint16_t *dst = a.sym + (a.out_off[row] - a.base);

	InfReader R(src, n, lane);
	if constexpr (BITS)
		R.drop(sh);
	uint32_t pos = 0;                                // symbols out so far (uniform), <= cap

	// symbols [p, p + length) from `offset` back, the whole wavefront: the source of symbol k is p - offset + (k mod offset),
	// which lies in front of p whatever the overlap; in front of the row's start it is a marker (p - offset + k >= -claim:
	// the caller has checked)
	auto copy = [&](uint32_t p, uint32_t length, uint32_t offset) {
		for (uint32_t k = lane; k < length; k += 64) {
			const int64_t s = (int64_t)p + (k % offset) - offset;
			const uint16_t v = s < 0 ? (uint16_t)(CARRY_MARK | (uint32_t)(CARRY_WINDOW + s)) : L.ring[(uint32_t)s & (CARRY_WINDOW - 1)];
			L.ring[(p + k) & (CARRY_WINDOW - 1)] = v;
			dst[p + k] = v;
		}
	};

	// the literals of a window's lanes in `mask`: lane's byte at its position
	auto put_literals = [&](uint64_t mask, uint32_t p, uint32_t byte) {
		if ((mask >> lane) & 1) {
			L.ring[p & (CARRY_WINDOW - 1)] = (uint16_t)(byte & 0xff);
			dst[p] = (uint16_t)(byte & 0xff);
		}
	};

	// ---- window decode: hd_inflate_size.hpp's, with the tokens' symbols placed.  Returns 0 = one token through the scalar
	// path, 2 = error (st set).
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
			const InfSpec s0 = spec_token(L, bl0, ws0, ws1, ws2), s1 = spec_token(L, bl0 + 64, ws2, ws3, ws4);
			uint32_t wb, wm;
			uint64_t real0, real1;
			window_walk(s0.walk, s1.walk, wb, real0, real1, wm);
			if (real0 == 0)
				break;                                     // the token at B is not for a window: scalar path
			const uint32_t scn = wave_incl_scan(sel(real0, s0.outlen, 0u) | (sel(real1, s1.outlen, 0u) << 16));
			const uint32_t tot = readlane(scn, 63);
			const uint32_t total = (tot & 0xffff) + (tot >> 16);
			if (total > cap - pos) {
				st_out = HD_INSUFFICIENT_SPACE;            // more than the table states
				result = 2;
				break;
			}
			const uint32_t opos0 = pos + (scn & 0xffff) - s0.outlen;
			const uint32_t opos1 = pos + (scn >> 16) + (tot & 0xffff) - s1.outlen;
			const uint64_t len0 = real0 & s0.is_len, len1 = real1 & s1.is_len;
			if (pos < CARRY_WINDOW) {
				// further back than the table states for this row: only this early can it be
				const uint64_t far0 = __ballot(opos0 < s0.offset && s0.offset - opos0 > claim);
				const uint64_t far1 = __ballot(opos1 < s1.offset && s1.offset - opos1 > claim);
				if ((far0 & len0) | (far1 & len1)) {
					st_out = HD_BAD_DATA;
					result = 2;
					break;
				}
			}
			// The tokens in stream order: the literals between two matches a lane each, a match by the whole wavefront.  The
			// order is kept strictly -- the ring is exactly as long as the longest distance, so a literal placed ahead of
			// its turn would land on the slot of a byte that a match 32768 - k in front of it still has to read.
			uint64_t lit0 = real0 & s0.is_lit, lit1 = real1 & s1.is_lit;
			for (uint64_t m = len0; m; m &= m - 1) {
				const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1;
				put_literals(lit0 & ((1ull << l) - 1), opos0, s0.length);
				lit0 &= ~((1ull << l) - 1);
				copy(readlane(opos0, l), readlane(s0.length, l), readlane(s0.offset, l));
			}
			put_literals(lit0, opos0, s0.length);
			for (uint64_t m = len1; m; m &= m - 1) {
				const uint32_t l = (uint32_t)__ffsll((unsigned long long)m) - 1;
				put_literals(lit1 & ((1ull << l) - 1), opos1, s1.length);
				lit1 &= ~((1ull << l) - 1);
				copy(readlane(opos1, l), readlane(s1.length, l), readlane(s1.offset, l));
			}
			put_literals(lit1, opos1, s1.length);
			pos += total;
			B += wb;
			if (wm & 64)
				break;                                     // the walk stopped in front of a long codeword or the end of the block
		}
		R.seek_bit(B);
		return result;
	};

	int32_t st = HD_OK;
	bool static_loaded = false;
	for (;;) {
		R.refill();
		lds_p0 = 0xfffffff0u;                     // header parsing reuses the LDS behind L.comp
		const uint32_t bfinal = (uint32_t)R.bb & 1;
		const uint32_t btype = ((uint32_t)R.bb >> 1) & 3;
		R.drop(3);

		if (btype == 0) {
			// ---- stored: the bytes are symbols ------------
			const int64_t cbits = (R.consumed_bits() + 7) & ~(int64_t)7;
			if (cbits > 8 * (int64_t)n) { st = HD_BAD_DATA; break; }
			uint32_t ip = (uint32_t)(cbits >> 3);
			if (n - ip < 4) { st = HD_BAD_DATA; break; }
			R.seek_byte(ip);
			R.refill();
			const uint32_t len = (uint32_t)R.bb & 0xffff, nlen = ((uint32_t)R.bb >> 16) & 0xffff;
			ip += 4;
			if (len != (~nlen & 0xffff)) { st = HD_BAD_DATA; break; }
			if (len > n - ip) { st = HD_BAD_DATA; break; }
			if (len > cap - pos) { st = HD_INSUFFICIENT_SPACE; break; }
			for (uint32_t k = lane; k < len; k += 64) {
				const uint16_t v = src[ip + k];
				L.ring[(pos + k) & (CARRY_WINDOW - 1)] = v;
				dst[pos + k] = v;
			}
			pos += len;
			R.seek_byte(ip + len);
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

			// ---- symbol loop ----------------------------------------------
			for (;;) {
				if (uniform(run_windows(st)))
					break;
				// one token through the fully checked scalar path (stream edges, long codes, end of block): the size pass's copy
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
					if (pos == cap) { st = HD_INSUFFICIENT_SPACE; break; }
					if (lane == 0) {
						L.ring[pos & (CARRY_WINDOW - 1)] = (uint16_t)(e >> 16);
						dst[pos] = (uint16_t)(e >> 16);
					}
					pos++;
					continue;
				}
				if (kind == K_EOB)
					break;
				const uint32_t eb = (e >> 4) & 15;
				const uint32_t length = (e >> 16) + ((uint32_t)R.bb & ((1u << eb) - 1));
				R.drop(eb);
				if (length > cap - pos) { st = HD_INSUFFICIENT_SPACE; break; }
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
				if (offset > pos && offset - pos > claim) { st = HD_BAD_DATA; break; }       // further back than the table states
				copy(pos, length, offset);
				pos += length;
			}
			if (st != HD_OK)
				break;
		}
		if (bfinal)
			break;
		if constexpr (BITS) {
			if (R.consumed_bits() >= (int64_t)end_bits)
				break;                                // the row's last bit is used -- or passed: bad data below
		} else {
			if (R.consumed_bits() <= 8 * (int64_t)n && R.consumed_bits() + 7 >= 8 * (int64_t)n)
				break;                                    // the flush rule: every input byte is used
			if (R.consumed_bits() > 8 * (int64_t)n + 64) { st = HD_BAD_DATA; break; }
		}
	}
	if (st == HD_OK && R.consumed_bits() > (BITS ? (int64_t)end_bits : 8 * (int64_t)n))
		st = HD_BAD_DATA;
	if (lane == 0) {
		a.out_len[row] = st == HD_OK ? pos : 0u;
		a.status[row] = st;
	}
}

#undef HD_ROWS_DECODE_KERNEL
#undef HD_ROWS_DECODE_ARGS
#undef HD_ROWS_DECODE_BITS
