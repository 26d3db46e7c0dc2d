// scratch_check.cpp -- 7bgzf_amd/csrc/hd_scratch.hpp held to what hd_api.hip needs of it, on the CPU (tests/test_host_scratch.py
// builds this with -fsanitize=address,undefined).  Every layout's columns are stated here a second time, as (type, element
// count) with the counts the kernels were given before the header existed -- cover[n + 1], nc = (ncand + 3) & ~3, the tiles
// of a scan of n -- and for every size: the counting walk and the placing walk end at the same byte; every column is aligned
// to its type over a 16-aligned base; the columns are disjoint (but for the one stated overlay) and inside bytes(); a pattern
// written through every column, at its stated count, into a heap buffer of exactly bytes() reads back intact.  No HIP,
// nothing of the library: the header alone.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "hd_scratch.hpp"

namespace {

int g_bad = 0, g_layouts = 0;
#define CHECK(cond, ...)                                                              \
	do {                                                                          \
		if (!(cond)) {                                                        \
			g_bad++;                                                      \
			fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
			fprintf(stderr, __VA_ARGS__);                                 \
			fputc('\n', stderr);                                          \
		}                                                                     \
	} while (0)

enum { PLAIN = 0, UNDER = 1, OVER = 2 };         // UNDER and OVER columns may share bytes: OVER is written once UNDER is dead
struct Col {
	const char *name;
	uint8_t *p;
	size_t width, count;                     // bytes per element (its alignment too), elements the kernels use
	int lay;
};
template <class T> Col col(const char *name, T *p, size_t count, int lay = PLAIN) { return { name, (uint8_t *)p, sizeof(T), count, lay }; }
// the eight words at the head of a buffer
template <class W> Col words(W *w)
{
	static_assert(sizeof(W) == 64 && alignof(W) == 8, "eight u64");
	return { "words", (uint8_t *)w, 8, 8, PLAIN };
}

size_t tiles(size_t n) { return (n + 2047) / 2048; }     // hd::SCAN_TILE elements a tile

uint64_t value(size_t k, size_t i) { return 0x9e3779b97f4a7c15ull * (k + 1) + i * 0x01000193u + k; }
void fill(const Col &c, size_t k)
{
	for (size_t i = 0; i < c.count; i++) {
		const uint64_t v = value(k, i);
		memcpy(c.p + i * c.width, &v, c.width);                  // (little endian: the low bytes)
	}
}
void verify(const char *what, const Col &c, size_t k)
{
	for (size_t i = 0; i < c.count; i++) {
		const uint64_t v = value(k, i);
		if (memcmp(c.p + i * c.width, &v, c.width)) {
			CHECK(false, "%s: column %s entry %zu was overwritten", what, c.name, i);
			return;
		}
	}
}

std::string fmt(const char *f, ...)
{
	char s[160];
	va_list ap;
	va_start(ap, f);
	vsnprintf(s, sizeof s, f, ap);
	va_end(ap);
	return s;
}

// L(base, args...) against its columns as `stated` here
template <class L, class Stated, class... A> void check(const std::string &name, Stated stated, A... a)
{
	const char *what = name.c_str();
	const size_t bytes = L::bytes(a...);
	uint8_t *buf = (uint8_t *)malloc(bytes);                     // exactly bytes(): a write past it is ASan's to report
	CHECK(buf && ((uintptr_t)buf & 15) == 0, "malloc gave a base that is not 16-aligned");
	const L t(buf, a...);
	CHECK(t.c.bytes() == bytes, "%s: the counting walk ends at %zu, the placing walk at %zu", what, bytes, t.c.bytes());
	const std::vector<Col> cols = stated(t);
	for (const Col &c : cols) {
		if (!c.count)
			continue;
		CHECK(c.p != nullptr, "%s: column %s is not there", what, c.name);
		if (!c.p)
			return free(buf);
		const size_t off = (size_t)(c.p - buf);
		CHECK(off % c.width == 0, "%s: column %s at %zu is not aligned to %zu", what, c.name, off, c.width);
		CHECK(c.p >= buf && off + c.count * c.width <= bytes, "%s: column %s [%zu, %zu) leaves the buffer", what, c.name, off,
		      off + c.count * c.width);
		for (const Col &d : cols)
			if (&d < &c && d.count && !(c.lay + d.lay == UNDER + OVER))
				CHECK(c.p + c.count * c.width <= d.p || d.p + d.count * d.width <= c.p, "%s: columns %s and %s overlap", what, d.name,
				      c.name);
	}
	if (g_bad)
		return free(buf);                                        // (no writes through a layout that is already wrong)
	for (size_t k = 0; k < cols.size(); k++)
		if (cols[k].lay != OVER)
			fill(cols[k], k);
	for (size_t k = 0; k < cols.size(); k++)
		if (cols[k].lay != OVER)
			verify(what, cols[k], k);
	for (size_t k = 0; k < cols.size(); k++)
		if (cols[k].lay == OVER)
			fill(cols[k], k);
	for (size_t k = 0; k < cols.size(); k++)
		if (cols[k].lay != UNDER)
			verify(what, cols[k], k);
	free(buf);
	g_layouts++;
}

void check_all(size_t n)
{
	// frame_table: p_off u64 | p_len, verdict, used, chk u32
	check<hd::FrameTable>(fmt("FrameTable(n=%zu)", n), [&](const hd::FrameTable &t) { return std::vector<Col>{
		col("p_off", t.p_off, n), col("p_len", t.p_len, n),
		col("verdict", t.verdict, n), col("used", t.used, n), col("chk", t.chk, n) }; }, n);
	// the index's first buffer: sum[8] | (the stream indexes: the header's [8]) | scan tiles | tile_off | bitmap | tile_cnt
	for (int hdr = 0; hdr < 2; hdr++)
		for (size_t nwords : { n, 4 * n - 1 }) {
			const size_t ntb = n;
			check<hd::IndexBitmap>(fmt("IndexBitmap(ntb=%zu nwords=%zu header=%d)", ntb, nwords, hdr), [&](const hd::IndexBitmap &t) { return std::vector<Col>{
					words(t.w), col("header", t.header, hdr ? 8 : 0), col("tiles", t.tiles, tiles(ntb)),
					col("tile_off", t.tile_off, ntb), col("bitmap", t.bitmap, nwords), col("tile_cnt", t.tile_cnt, ntb) }; },
				ntb, nwords, hdr != 0);
		}
	// ... and its candidate buffer: scan tiles | pos | succ[2] (later: rank) | mark | hdr | total, or (a stream index)
	// | mark | in_used | out_size | status | stop (| reach: the carry index)
	for (int kind = 0; kind < 3; kind++)
		for (size_t max_rows : { (size_t)0, (size_t)1, n, (size_t)5000 }) {
			const size_t ncand = n, nc = (ncand + 3) & ~(size_t)3, nm = kind == 0 ? nc : 0, ns = kind == 0 ? 0 : nc;
			check<hd::IndexCand>(fmt("IndexCand(ncand=%zu max_rows=%zu kind=%d)", ncand, max_rows, kind), [&](const hd::IndexCand &t) { return std::vector<Col>{
					col("tiles", t.tiles, tiles(ncand) + tiles(max_rows)), col("pos", t.pos, nc), col("succ0", t.succ0, nc, UNDER),
					col("succ1", t.succ1, nc, UNDER), col("rank", t.rank, nc, OVER), col("mark", t.mark, nc), col("hdr", t.hdr, nm),
					col("total", t.total, nm), col("used", t.used, ns), col("osize", t.osize, ns), col("pstat", t.pstat, ns),
					col("stop", t.stop, ns), col("reach", t.reach, kind == 2 ? nc : 0) }; },
				ncand, max_rows, (hd::IndexKind)kind);
		}
	// the range call: sum[8] | scan tiles | cover_scan[n + 1] | rank, scratch_off, c_in_off, c_out_off [n] | q_from, piece_off [nq] |
	// cover[n + 1] | sel, sel_size, c_in_len, c_out_cap, c_crc_want, c_member, c_out_len, c_crc, c_status [n] | q_pieces, q_first [nq]
	for (size_t nq : { (size_t)1, n, n + 1, n + 2, (size_t)2049 })
		check<hd::RangeTables>(fmt("RangeTables(n=%zu nq=%zu)", n, nq), [&](const hd::RangeTables &t) { return std::vector<Col>{
				words(t.w), col("tiles", t.tiles, tiles(n + 1 > nq ? n + 1 : nq)), col("cover_scan", t.cover_scan, n + 1),
				col("rank", t.rank, n), col("scratch_off", t.scratch_off, n), col("c_in_off", t.c_in_off, n),
				col("c_out_off", t.c_out_off, n), col("q_from", t.q_from, nq), col("piece_off", t.piece_off, nq),
				col("cover", t.cover, n + 1), col("sel", t.sel, n), col("sel_size", t.sel_size, n), col("c_in_len", t.c_in_len, n),
				col("c_out_cap", t.c_out_cap, n), col("c_crc_want", t.c_crc_want, n), col("c_member", t.c_member, n),
				col("c_out_len", t.c_out_len, n), col("c_crc", t.c_crc, n), col("c_status", t.c_status, n),
				col("q_pieces", t.q_pieces, nq), col("q_first", t.q_first, nq) }; },
			n, nq);
	// the fold: sum[8] | scan tiles | prefix [n]
	check<hd::FoldScratch>(fmt("FoldScratch(n=%zu)", n), [&](const hd::FoldScratch &t) { return std::vector<Col>{
	words(t.w), col("tiles", t.tiles, tiles(n)), col("prefix", t.prefix, n) }; }, n);
	// the encode window: sum[8] | scan tiles | in_off, own_off, prefix [W] | in_len, out_len, crc, adler, status [W]
	check<hd::EncodeWindow>(fmt("EncodeWindow(W=%zu)", n), [&](const hd::EncodeWindow &t) { return std::vector<Col>{
			words(t.w), col("tiles", t.tiles, tiles(n)), col("in_off", t.in_off, n), col("own_off", t.own_off, n),
			col("prefix", t.prefix, n), col("in_len", t.in_len, n), col("out_len", t.out_len, n), col("crc", t.crc, n),
			col("adler", t.adler, n), col("status", t.status, n) }; }, n);
	// the decoders: sum[8] | the header's [8], where the rows end [2], the group's record [4] | scan tiles | prefix [n] |
	// out_len, check, status [n], and the decode by chunk table's own in_off, out_off | in_len, out_size [n]
	for (int own = 0; own < 2; own++)
		check<hd::DecodeScratch>(fmt("DecodeScratch(n=%zu own_table=%d)", n, own), [&](const hd::DecodeScratch &t) { return std::vector<Col>{
				words(t.w), col("header", t.header, 8), col("ends", t.ends, 2), col("group", t.group, 4), col("tiles", t.tiles, tiles(n)),
				col("prefix", t.prefix, n), col("out_len", t.out_len, n), col("chk", t.chk, n), col("status", t.status, n),
				col("in_off", t.in_off, own ? n : 0), col("out_off", t.out_off, own ? n : 0), col("in_len", t.in_len, own ? n : 0),
				col("out_size", t.out_size, own ? n : 0) }; },
			n, own != 0);
	// the marker path: symbols, (2 * gbytes + 15) & ~15 bytes of them | the check's pieces: off, prefix u64[np], scan tiles |
	// len, check u32[np] | + 16
	for (uint64_t gbytes : { (uint64_t)n, (uint64_t)n * 37 + 1 }) {
		const size_t np = n, nsym = (size_t)(((2 * gbytes + 15) & ~(uint64_t)15) / 2);
		check<hd::MarkerScratch>(fmt("MarkerScratch(gbytes=%llu np=%zu)", (unsigned long long)gbytes, np), [&](const hd::MarkerScratch &t) { return std::vector<Col>{
				col("sym", t.sym, nsym), col("off", t.off, np), col("prefix", t.prefix, np), col("tiles", t.tiles, tiles(np)),
				col("len", t.len, np), col("chk", t.chk, np), col("slack", t.slack, 16) }; },
			gbytes, np);
	}
	// the row table in d_meta: in_off, out_off u64[n] | in_len, out_size u32[n] (carry: | reach u32[n]) | + 64
	for (int carry = 0; carry < 2; carry++)
		check<hd::RowTable>(fmt("RowTable(n=%zu carry=%d)", n, carry), [&](const hd::RowTable &t) { return std::vector<Col>{
				col("in_off", t.in_off, n), col("out_off", t.out_off, n), col("in_len", t.in_len, n), col("out_size", t.out_size, n),
				col("reach", t.reach, carry ? n : 0), col("slack", t.slack, 64) }; },
			n, carry != 0);
}

} // namespace

int main()
{
	static const size_t ns[] = { 1, 2, 3, 4, 5, 63, 64, 65, 2047, 2048, 2049, 65536 };
	for (size_t n : ns)
		check_all(n);
	printf("scratch_check: %zu sizes, %d layouts, %d bad\n", sizeof ns / sizeof ns[0], g_layouts, g_bad);
	return g_bad ? 1 : 0;
}
