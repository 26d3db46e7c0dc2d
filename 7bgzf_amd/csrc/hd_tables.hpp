// hd_tables.hpp -- the two per-block metadata tables of the host layer (hd_api.hip), each layout stated once.
//
// A table is `n` blocks in columns, one column after the other, over a raw buffer: a pinned one on the host, a device one,
// or pinned memory the device sees.  Both sides of a copy use one layout, so a range of columns travels in one copy and
// lands at the offset it left from.  A column's offset is (its constant below) * n: the u64 columns' constants are
// multiples of 8, so they are 8-byte aligned over an 8-aligned base for every n, with no padding anywhere.
//
// Plain C++, no HIP: a host compiler builds it alone (tests/native/tables_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hd {

struct Span {                                // a run of whole columns: what one copy moves
	size_t off, bytes;
};

class TableBase {
protected:
	uint8_t *b;
	size_t n;
	template <class T> T *col(size_t per_block) const { return (T *)(b + per_block * n); }
	Span cols(size_t from, size_t to, size_t tail = 0) const { return { from * n, (to - from) * n + tail }; }

public:
	TableBase(void *base, size_t nblocks) : b((uint8_t *)base), n(nblocks) {}
	uint8_t *ptr(Span s) const { return b + s.off; }
};

// encode: in_off u64 | in_len, out_len, crc, status u32 | dst_off u64 | total u64 (one word, behind the columns)
class EncTable : public TableBase {
	enum : size_t { IN_OFF = 0, IN_LEN = 8, OUT_LEN = 12, CRC = 16, STATUS = 20, DST_OFF = 24, TOTAL = 32 };
	static_assert(IN_OFF % 8 == 0 && DST_OFF % 8 == 0 && TOTAL % 8 == 0, "a u64 column must start on 8 bytes for every n");

public:
	using TableBase::TableBase;
	static constexpr size_t bytes(size_t n) { return TOTAL * n + 8; }
	uint64_t *in_off() const { return col<uint64_t>(IN_OFF); }
	uint32_t *in_len() const { return col<uint32_t>(IN_LEN); }
	uint32_t *out_len() const { return col<uint32_t>(OUT_LEN); }
	uint32_t *crc() const { return col<uint32_t>(CRC); }
	int32_t *status() const { return col<int32_t>(STATUS); }
	uint64_t *dst_off() const { return col<uint64_t>(DST_OFF); }         // where the gather puts each member
	uint64_t *total() const { return col<uint64_t>(TOTAL); }             // ... and the bytes it wrote
	Span inputs() const { return cols(IN_OFF, OUT_LEN); }                // host to device: in_off, in_len
	Span results() const { return cols(OUT_LEN, DST_OFF); }              // back: out_len, crc, status
	Span results_placed() const { return cols(OUT_LEN, TOTAL, 8); }      // ... with dst_off and total (the pipe)
};

// decode: in_off, out_off u64 | in_len, out_cap, out_len, status, crc u32 (crc last: who wants none copies none)
class DecTable : public TableBase {
	enum : size_t { IN_OFF = 0, OUT_OFF = 8, IN_LEN = 16, OUT_CAP = 20, OUT_LEN = 24, STATUS = 28, CRC = 32, END = 36 };
	static_assert(IN_OFF % 8 == 0 && OUT_OFF % 8 == 0, "a u64 column must start on 8 bytes for every n");

public:
	using TableBase::TableBase;
	static constexpr size_t bytes(size_t n) { return END * n; }
	uint64_t *in_off() const { return col<uint64_t>(IN_OFF); }
	uint64_t *out_off() const { return col<uint64_t>(OUT_OFF); }
	uint32_t *in_len() const { return col<uint32_t>(IN_LEN); }
	uint32_t *out_cap() const { return col<uint32_t>(OUT_CAP); }
	uint32_t *out_len() const { return col<uint32_t>(OUT_LEN); }
	int32_t *status() const { return col<int32_t>(STATUS); }
	uint32_t *crc() const { return col<uint32_t>(CRC); }
	Span inputs() const { return cols(IN_OFF, OUT_LEN); }                // host to device: in_off, out_off, in_len, out_cap
	Span results() const { return cols(OUT_LEN, CRC); }                  // back: out_len, status
	Span results_crc() const { return cols(OUT_LEN, END); }              // ... and crc
};

} // namespace hd
