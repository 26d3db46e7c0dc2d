// hd_scratch.hpp -- the scratch layouts of the device-resident calls (hd_api.hip), each stated once.
//
// A layout is a struct whose members are its columns, each declared with the take<T>(count) that places it: members are
// initialised in the order declared, so the declaration is the layout, and the constructor is the one function that lays it
// out.  Over no base the same walk only counts -- bytes() is that -- so the size asked of a buffer and the pointers into
// it cannot disagree.  take<T> aligns to alignof(T): a buffer may hold a few bytes of padding.  The words at the head of
// a buffer, through which kernels and the host hand verdicts, are structs with named members; the kernels get plain
// pointers to them.
//
// Plain C++, no HIP: a host compiler builds it alone (tests/native/scratch_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace hd {

class Carve {
	uint8_t *b;
	size_t at = 0;

public:
	explicit Carve(void *base) : b((uint8_t *)base) {}
	template <class T> T *take(size_t count)
	{
		at = (at + alignof(T) - 1) & ~(alignof(T) - 1);
		T *p = b ? (T *)(b + at) : nullptr;
		at += count * sizeof(T);
		return p;
	}
	// an overlay: T[count] in the place of what was taken since `from` (a bytes() of before); the carve goes on behind the longer
	template <class T> T *over(size_t from, size_t count)
	{
		Carve o(b);
		o.at = from;
		T *p = o.take<T>(count);
		at = at > o.at ? at : o.at;
		return p;
	}
	size_t bytes() const { return at; }
};

template <class L> struct Layout {
	Carve c;
	explicit Layout(void *base) : c(base) {}
	template <class... A> static size_t bytes(A... a) { return L(nullptr, a...).c.bytes(); }
};

constexpr size_t SCRATCH_SCAN_TILE = 2048;   // hd::SCAN_TILE (hd_compact.hpp): hd_api.hip holds the two equal
inline size_t scan_tiles(size_t n) { return (n + SCRATCH_SCAN_TILE - 1) / SCRATCH_SCAN_TILE; }

/* ---- the words at the head of a buffer: 64 bytes each ---- */

// the member index and both stream indexes (d_index); hipdeflate_verify_members_dev uses `first` alone
struct IndexWords {
	uint64_t rows, out_bytes, end_offset, status;    // the summary: the verdict kernels write it from `rows` on (before: the rank scan's total)
	uint64_t ncand;                                  // the flag pass's total
	uint64_t last;                                   // k_stream_rows: the last row's candidate
	uint32_t first, pad;                             // the lowest row at fault: the carry's reach rule, the verify's bad member
	uint64_t spare;
};
// the range call (d_range)
struct RangeWords {
	uint64_t out_bytes, pieces, cover_total, nselected, sel_bytes, bad_member;
	uint32_t nrefused, pad0;
	uint32_t bad_row, pad1;                          // the lowest bad row of the selection (0xffffffff: none)
};
// the stream calls (d_stream): the encode window, the three decoders, the fold
struct StreamVerdict {
	uint32_t check;                                  // the folded check, running (0 / 1 before the first fold)
	uint32_t fault;                                  // the lowest table fault (the encode: the window's lowest bad chunk); 0xffffffff: none
	uint32_t mismatch;                               // the trailer disagrees
	uint32_t bad;                                    // the lowest bad row; 0xffffffff: none
};
struct StreamWords {
	uint64_t total;                                  // the encode: the window's bytes out
	uint64_t fold[3];                                // fold_launch: the parts' bytes, two accumulators
	StreamVerdict v;
	uint64_t spare[2];
};
static_assert(sizeof(IndexWords) == 64 && sizeof(RangeWords) == 64 && sizeof(StreamWords) == 64, "eight u64 at the head of a buffer");

/* ---- the layouts ---- */

// the payload table of one framed call (Ctx::frame): n members
struct FrameTable : Layout<FrameTable> {
	FrameTable(void *base = nullptr, size_t n_ = 0) : Layout(base), n(n_) {}
	size_t n;
	uint64_t *p_off = c.take<uint64_t>(n);
	uint32_t *p_len = c.take<uint32_t>(n), *used = c.take<uint32_t>(n), *chk = c.take<uint32_t>(n);
	int32_t *verdict = c.take<int32_t>(n);
};

// d_index: the flag pass over ntb tiles of nwords bitmap words.  header: stream_open's eight words (the stream indexes)
struct IndexBitmap : Layout<IndexBitmap> {
	IndexBitmap(void *base = nullptr, size_t ntb_ = 0, size_t nwords_ = 0, bool header_ = false)
		: Layout(base), ntb(ntb_), nwords(nwords_), nhdr(header_ ? 8 : 0) {}
	size_t ntb, nwords, nhdr;
	IndexWords *w = c.take<IndexWords>(1);
	uint64_t *header = c.take<uint64_t>(nhdr), *tiles = c.take<uint64_t>(scan_tiles(ntb)), *tile_off = c.take<uint64_t>(ntb);
	uint64_t *bitmap = c.take<uint64_t>(nwords);
	uint32_t *tile_cnt = c.take<uint32_t>(ntb);
};

// d_cand: ncand candidates in columns of nc, and the tiles of two scans, of ncand and of max_rows elements.  The successor
// tables are dead when the rank scan runs: rank lies over them.  INDEX_ANY (members that state no length) is INDEX_MEMBERS
// with every candidate's class and the columns of its sizing subset; its subset scan runs before the successor tables are
// written, into rank as well.
enum IndexKind { INDEX_MEMBERS, INDEX_STREAM, INDEX_CARRY, INDEX_BLOCKS, INDEX_ANY };
struct IndexCand : Layout<IndexCand> {
	IndexCand(void *base = nullptr, size_t ncand = 0, size_t max_rows = 0, IndexKind kind = INDEX_MEMBERS)
		: Layout(base), nc((ncand + 3) & ~(size_t)3), ntiles(scan_tiles(ncand) + scan_tiles(max_rows)),
		  nm(kind == INDEX_MEMBERS || kind == INDEX_ANY ? nc : 0), ns(kind == INDEX_MEMBERS || kind == INDEX_ANY ? 0 : nc),
		  nr(kind == INDEX_CARRY || kind == INDEX_BLOCKS ? nc : 0), na(kind == INDEX_ANY ? nc : 0) {}
	size_t nc, ntiles, nm, ns, nr, na;
	uint64_t *tiles = c.take<uint64_t>(ntiles), *pos = c.take<uint64_t>(nc);
	size_t succ_at = c.bytes();
	uint32_t *succ0 = c.take<uint32_t>(nc), *succ1 = c.take<uint32_t>(nc);
	uint64_t *rank = c.over<uint64_t>(succ_at, nc);
	uint32_t *mark = c.take<uint32_t>(nc);
	uint32_t *hdr = c.take<uint32_t>(nm), *total = c.take<uint32_t>(nm);                                         // INDEX_MEMBERS, INDEX_ANY
	uint32_t *used = c.take<uint32_t>(ns), *osize = c.take<uint32_t>(ns), *stop = c.take<uint32_t>(ns);          // both stream indexes
	int32_t *pstat = c.take<int32_t>(ns);
	uint32_t *reach = c.take<uint32_t>(nr);                                                                      // INDEX_CARRY, INDEX_BLOCKS
	uint32_t *cls = c.take<uint32_t>(na), *tosize = c.take<uint32_t>(na), *sub = c.take<uint32_t>(na);           // INDEX_ANY
	uint32_t *asize = c.take<uint32_t>(na);
	int32_t *astat = c.take<int32_t>(na);
};

// d_blocks, the block index's merge (hd_blocks.hpp): the np pieces of the chain in rank order, and the rows they merge into
// (np at the most, and one entry behind the last row: the chain's end)
struct BlockPieces : Layout<BlockPieces> {
	BlockPieces(void *base, size_t np_) : Layout(base), np(np_) {}
	size_t np;
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(np)), *p_out = c.take<uint64_t>(np), *before = c.take<uint64_t>(np);
	uint64_t *h_pos = c.take<uint64_t>(np + 1), *h_out = c.take<uint64_t>(np + 1);
	uint32_t *p_size = c.take<uint32_t>(np), *start = c.take<uint32_t>(np);
};

// d_range: n members, nq queries
struct RangeTables : Layout<RangeTables> {
	RangeTables(void *base, size_t n_, size_t nq_) : Layout(base), n(n_), nq(nq_) {}
	size_t n, nq;
	RangeWords *w = c.take<RangeWords>(1);
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(n + 1 > nq ? n + 1 : nq)), *cover_scan = c.take<uint64_t>(n + 1);
	uint64_t *rank = c.take<uint64_t>(n), *scratch_off = c.take<uint64_t>(n), *c_in_off = c.take<uint64_t>(n);
	uint64_t *c_out_off = c.take<uint64_t>(n), *q_from = c.take<uint64_t>(nq), *piece_off = c.take<uint64_t>(nq);
	uint32_t *cover = c.take<uint32_t>(n + 1), *sel = c.take<uint32_t>(n), *sel_size = c.take<uint32_t>(n);
	uint32_t *c_in_len = c.take<uint32_t>(n), *c_out_cap = c.take<uint32_t>(n), *c_crc_want = c.take<uint32_t>(n);
	uint32_t *c_member = c.take<uint32_t>(n), *c_out_len = c.take<uint32_t>(n), *c_crc = c.take<uint32_t>(n);
	int32_t *c_status = c.take<int32_t>(n);
	uint32_t *q_pieces = c.take<uint32_t>(nq), *q_first = c.take<uint32_t>(nq);
};

// d_stream, hipdeflate_check_combine_dev: the fold of n parts
struct FoldScratch : Layout<FoldScratch> {
	FoldScratch(void *base, size_t n_) : Layout(base), n(n_) {}
	size_t n;
	StreamWords *w = c.take<StreamWords>(1);
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(n)), *prefix = c.take<uint64_t>(n);
};

// d_stream, hipdeflate_stream_deflate_dev: a window of n chunks
struct EncodeWindow : Layout<EncodeWindow> {
	EncodeWindow(void *base, size_t n_) : Layout(base), n(n_) {}
	size_t n;
	StreamWords *w = c.take<StreamWords>(1);
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(n)), *in_off = c.take<uint64_t>(n), *own_off = c.take<uint64_t>(n);
	uint64_t *prefix = c.take<uint64_t>(n);
	uint32_t *in_len = c.take<uint32_t>(n), *out_len = c.take<uint32_t>(n), *crc = c.take<uint32_t>(n), *adler = c.take<uint32_t>(n);
	int32_t *status = c.take<int32_t>(n);
};

// d_stream, the three decoders: n rows.  own_table: the decode by chunk table makes its row table here
struct DecodeScratch : Layout<DecodeScratch> {
	DecodeScratch(void *base, size_t n_, bool own_table) : Layout(base), n(n_), nt(own_table ? n_ : 0) {}
	size_t n, nt;
	StreamWords *w = c.take<StreamWords>(1);
	uint64_t *header = c.take<uint64_t>(8);          // stream_open's eight words
	uint64_t *ends = c.take<uint64_t>(2);            // k_stream_check_rows: where the rows end, in the stream and in the output
	uint64_t *group = c.take<uint64_t>(4);           // k_carry_group's record
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(n)), *prefix = c.take<uint64_t>(n);
	uint32_t *out_len = c.take<uint32_t>(n), *chk = c.take<uint32_t>(n);
	int32_t *status = c.take<int32_t>(n);
	uint64_t *in_off = c.take<uint64_t>(nt), *out_off = c.take<uint64_t>(nt);
	uint32_t *in_len = c.take<uint32_t>(nt), *out_size = c.take<uint32_t>(nt);
};

// d_stream_slots, the carry decode's marker path: a group of gbytes output bytes as 16-bit symbols (a multiple of 16 bytes
// of them), its check in np pieces, and the 16 bytes that every data buffer of the library has behind its end
struct MarkerScratch : Layout<MarkerScratch> {
	MarkerScratch(void *base, uint64_t gbytes, size_t np_) : Layout(base), nsym((size_t)((gbytes + 7) & ~(uint64_t)7)), np(np_) {}
	size_t nsym, np;
	uint16_t *sym = c.take<uint16_t>(nsym);
	uint64_t *off = c.take<uint64_t>(np), *prefix = c.take<uint64_t>(np), *tiles = c.take<uint64_t>(scan_tiles(np));
	uint32_t *len = c.take<uint32_t>(np), *chk = c.take<uint32_t>(np);
	uint8_t *slack = c.take<uint8_t>(16);
};

// d_stream, hipdeflate_stream_windows_dev: the verdict words and the tiles of the scan of n reach values
struct WindowScratch : Layout<WindowScratch> {
	WindowScratch(void *base, size_t n_) : Layout(base), n(n_) {}
	size_t n;
	StreamWords *w = c.take<StreamWords>(1);
	uint64_t *tiles = c.take<uint64_t>(scan_tiles(n));
};

// d_stream, hipdeflate_stream_read_ranges_dev (hd_seek.hpp): the check of a table of n rows, and the selected rows' compacted
// tables with the row decoder's verdicts (at most n rows are selected; the queries' tables are a RangeTables in d_range)
struct SeekTables : Layout<SeekTables> {
	SeekTables(void *base, size_t n_) : Layout(base), n(n_) {}
	size_t n;
	StreamWords *w = c.take<StreamWords>(1);
	uint64_t *header = c.take<uint64_t>(8);          // stream_open's eight words
	uint64_t *ends = c.take<uint64_t>(2);            // k_stream_check_rows / k_blocks_check_rows: where the rows end
	uint64_t *group = c.take<uint64_t>(4);           // k_carry_group's record
	uint64_t *c_in_off = c.take<uint64_t>(n), *c_out_off = c.take<uint64_t>(n), *c_win_off = c.take<uint64_t>(n);
	uint32_t *c_in_len = c.take<uint32_t>(n), *c_out_size = c.take<uint32_t>(n), *c_reach = c.take<uint32_t>(n);
	uint32_t *c_row_check = c.take<uint32_t>(n), *c_row = c.take<uint32_t>(n);
	uint32_t *out_len = c.take<uint32_t>(n), *crc = c.take<uint32_t>(n);
	int32_t *status = c.take<int32_t>(n);
};

// the row table that stream_index makes in d_meta for the host-buffer forms, and that they read back: n rows
struct RowTable : Layout<RowTable> {
	RowTable(void *base, size_t n_, bool carry) : Layout(base), n(n_), nr(carry ? n_ : 0) {}
	size_t n, nr;
	uint64_t *in_off = c.take<uint64_t>(n), *out_off = c.take<uint64_t>(n);
	uint32_t *in_len = c.take<uint32_t>(n), *out_size = c.take<uint32_t>(n), *reach = c.take<uint32_t>(nr);
	uint8_t *slack = c.take<uint8_t>(64);            // room behind the rows, as the table has always had
};

// the member table that hip_inflate_members makes in d_meta, and the inflate's answers on it: n members
struct MemberTables : Layout<MemberTables> {
	MemberTables(void *base, size_t n_) : Layout(base), n(n_) {}
	size_t n;
	uint64_t *in_off = c.take<uint64_t>(n), *out_off = c.take<uint64_t>(n);
	uint32_t *in_len = c.take<uint32_t>(n), *out_size = c.take<uint32_t>(n), *crc_want = c.take<uint32_t>(n);
	uint32_t *out_len = c.take<uint32_t>(n), *crc = c.take<uint32_t>(n);
	int32_t *status = c.take<int32_t>(n);
};

} // namespace hd
