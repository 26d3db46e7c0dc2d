// tables_check.cpp -- 7bgzf_amd/csrc/hd_tables.hpp held to what it states, on the CPU (tests/test_host_tables.py builds this
// with -fsanitize=address,undefined): for every n, every u64 column 8-aligned over an aligned base, the columns disjoint and
// inside bytes(n), each copy range exactly its columns, and a pattern written through every accessor into a heap buffer of
// exactly bytes(n) read back intact.  No HIP, nothing of the library: the header alone.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "hd_tables.hpp"

namespace {

struct Col {
	const char *name;
	size_t off, width, count;                // bytes from the base, bytes per entry, entries
	size_t end() const { return off + width * count; }
};

int g_bad = 0;
#define CHECK(cond, ...)                                                              \
	do {                                                                          \
		if (!(cond)) {                                                        \
			g_bad++;                                                      \
			fprintf(stderr, "FAIL %s:%d: %s -- ", __FILE__, __LINE__, #cond); \
			fprintf(stderr, __VA_ARGS__);                                 \
			fputc('\n', stderr);                                          \
		}                                                                     \
	} while (0)

template <class T> Col col(const char *name, const uint8_t *base, const T *p, size_t count)
{
	return { name, (size_t)((const uint8_t *)p - base), sizeof(T), count };
}

// the columns in the order of the layout: each starts where the one before ends, the last ends at bytes(n)
void check_columns(const char *table, size_t n, const std::vector<Col> &cols, size_t bytes)
{
	size_t at = 0;
	for (const Col &c : cols) {
		CHECK(c.off == at, "%s n=%zu: column %s at %zu, the one before ends at %zu", table, n, c.name, c.off, at);
		CHECK(c.width != 8 || c.off % 8 == 0, "%s n=%zu: u64 column %s at %zu", table, n, c.name, c.off);
		at = c.end();
	}
	CHECK(at == bytes, "%s n=%zu: columns end at %zu, bytes(n) = %zu", table, n, at, bytes);
}

// a copy range is exactly the columns first .. last
void check_span(const char *table, const char *what, size_t n, hd::Span s, const Col &first, const Col &last)
{
	CHECK(s.off == first.off && s.off + s.bytes == last.end(), "%s n=%zu: %s is [%zu, %zu), its columns %s..%s are [%zu, %zu)", table, n,
	      what, s.off, s.off + s.bytes, first.name, last.name, first.off, last.end());
}

// entry i of column k holds a value of its own (a stray write from another column or entry shows)
template <class T> void fill(T *p, size_t count, uint64_t k)
{
	for (size_t i = 0; i < count; i++)
		p[i] = (T)(0x9e3779b97f4a7c15ull * (k + 1) + i * 0x01000193u + k);
}
template <class T> void verify(const char *table, const char *name, size_t n, const T *p, size_t count, uint64_t k)
{
	for (size_t i = 0; i < count; i++)
		if (p[i] != (T)(0x9e3779b97f4a7c15ull * (k + 1) + i * 0x01000193u + k)) {
			CHECK(false, "%s n=%zu: column %s entry %zu was overwritten", table, n, name, i);
			return;
		}
}

void check_enc(size_t n)
{
	const size_t bytes = hd::EncTable::bytes(n);
	uint8_t *buf = (uint8_t *)malloc(bytes);                 // exactly bytes(n): a write past it is ASan's to report
	CHECK(((uintptr_t)buf & 7) == 0, "malloc gave an unaligned base");
	const hd::EncTable t(buf, n);
	const std::vector<Col> c = { col("in_off", buf, t.in_off(), n), col("in_len", buf, t.in_len(), n), col("out_len", buf, t.out_len(), n),
				     col("crc", buf, t.crc(), n), col("status", buf, t.status(), n), col("dst_off", buf, t.dst_off(), n),
				     col("total", buf, t.total(), 1) };
	check_columns("EncTable", n, c, bytes);
	check_span("EncTable", "inputs", n, t.inputs(), c[0], c[1]);
	check_span("EncTable", "results", n, t.results(), c[2], c[4]);
	check_span("EncTable", "results_placed", n, t.results_placed(), c[2], c[6]);
	CHECK(t.ptr(t.results()) == (uint8_t *)t.out_len(), "EncTable n=%zu: ptr(results) is not out_len", n);
	fill(t.in_off(), n, 0), fill(t.in_len(), n, 1), fill(t.out_len(), n, 2), fill(t.crc(), n, 3), fill(t.status(), n, 4);
	fill(t.dst_off(), n, 5), fill(t.total(), 1, 6);
	verify("EncTable", "in_off", n, t.in_off(), n, 0), verify("EncTable", "in_len", n, t.in_len(), n, 1);
	verify("EncTable", "out_len", n, t.out_len(), n, 2), verify("EncTable", "crc", n, t.crc(), n, 3);
	verify("EncTable", "status", n, t.status(), n, 4), verify("EncTable", "dst_off", n, t.dst_off(), n, 5);
	verify("EncTable", "total", n, t.total(), 1, 6);
	free(buf);
}

void check_dec(size_t n)
{
	const size_t bytes = hd::DecTable::bytes(n);
	uint8_t *buf = (uint8_t *)malloc(bytes);
	CHECK(((uintptr_t)buf & 7) == 0, "malloc gave an unaligned base");
	const hd::DecTable t(buf, n);
	const std::vector<Col> c = { col("in_off", buf, t.in_off(), n), col("out_off", buf, t.out_off(), n), col("in_len", buf, t.in_len(), n),
				     col("out_cap", buf, t.out_cap(), n), col("out_len", buf, t.out_len(), n), col("status", buf, t.status(), n),
				     col("crc", buf, t.crc(), n) };
	check_columns("DecTable", n, c, bytes);
	check_span("DecTable", "inputs", n, t.inputs(), c[0], c[3]);
	check_span("DecTable", "results", n, t.results(), c[4], c[5]);
	check_span("DecTable", "results_crc", n, t.results_crc(), c[4], c[6]);
	CHECK(t.ptr(t.results()) == (uint8_t *)t.out_len(), "DecTable n=%zu: ptr(results) is not out_len", n);
	fill(t.in_off(), n, 0), fill(t.out_off(), n, 1), fill(t.in_len(), n, 2), fill(t.out_cap(), n, 3), fill(t.out_len(), n, 4);
	fill(t.status(), n, 5), fill(t.crc(), n, 6);
	verify("DecTable", "in_off", n, t.in_off(), n, 0), verify("DecTable", "out_off", n, t.out_off(), n, 1);
	verify("DecTable", "in_len", n, t.in_len(), n, 2), verify("DecTable", "out_cap", n, t.out_cap(), n, 3);
	verify("DecTable", "out_len", n, t.out_len(), n, 4), verify("DecTable", "status", n, t.status(), n, 5);
	verify("DecTable", "crc", n, t.crc(), n, 6);
	free(buf);
}

} // namespace

int main()
{
	static const size_t ns[] = { 1, 2, 3, 5, 64, 65, 1024, 65536 };
	for (size_t n : ns) {
		check_enc(n);
		check_dec(n);
	}
	printf("tables_check: %zu sizes, %d bad\n", sizeof ns / sizeof ns[0], g_bad);
	return g_bad ? 1 : 0;
}
