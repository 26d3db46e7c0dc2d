"""The model of the ranged read (tests/range_read_model.py) held to what it restates: data[begin:end] of the file as
zlib decodes it, member by member.  Both kinds of offsets, the five member kinds, empty members in the middle, three EOF
blocks at the end, and every validity rule of include/hipdeflate.h, one case each.  No GPU."""
import zlib

import numpy as np
import pytest

import hdtest
import member_index_model as mm
import range_read_model as rm

KINDS = ["BC", "MZ", "IG1", "IG2", "MG"]


def raw_deflate(data, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def coded(kind, chunk, **kw):
    return mm.gz_member(kind, raw_deflate(chunk), zlib.crc32(chunk), len(chunk), **kw)


def gunzip_members(blob):
    """-> [(start offset, decoded bytes)] by zlib alone"""
    out, at = [], 0
    while at < len(blob):
        z = zlib.decompressobj(31)
        d = z.decompress(blob[at:])
        out.append((at, d))
        at = len(blob) - len(z.unused_data)
    return out


def mixed_file():
    """27 members of the five kinds, some named, empty ones at 5, 6 and 13, three EOF blocks at the end"""
    eof = hdtest.pkg().BGZF_EOF
    chunks = [bytes(hdtest.synth().text_like(50 + 131 * k, seed=k)) for k in range(24)]
    for k in (5, 6, 13):
        chunks[k] = b""
    parts = [coded(KINDS[k % 5], c, fname=b"f%d" % k if k % 3 == 0 else b"", fcomment=b"c" if k % 4 == 1 else b"") for k, c in enumerate(chunks)]
    return b"".join(parts) + eof * 3, b"".join(chunks)


@pytest.fixture(scope="module")
def mixed():
    blob, data = mixed_file()
    rows, status, end = mm.walk(blob)
    assert status == mm.OK and end == len(blob) and len(rows) == 27
    return blob, data, rows


def check_against_slices(rows, data, kind, begins, ends, spans_want):
    """spans_want[q] = (b, e) for an accepted query, None for a refused one"""
    p = rm.plan(rows, kind, begins, ends)
    at = 0
    for q, want in enumerate(spans_want):
        if want is None:
            assert p["q_status"][q] != 0 and p["q_len"][q] == 0, q
        else:
            b, e = want
            assert p["q_status"][q] == 0 and p["q_len"][q] == len(data[b:e]), (q, want)
            assert data[p["spans"][q][0]:p["spans"][q][1]] == data[b:e], (q, want)
        assert p["dst_off"][q] == at
        at += p["q_len"][q]
    assert p["out_bytes"] == at and p["nrefused"] == sum(1 for w in spans_want if w is None)
    # a member is selected exactly when some accepted query takes a byte that zlib says is its own
    owner = np.repeat(np.arange(len(rows)), [r[2] for r in rows])      # the member every decoded byte came from
    assert len(owner) == len(data)
    touched = set()
    for want in spans_want:
        if want is not None:
            touched.update(int(m) for m in np.unique(owner[want[0]:want[1]]))
    assert p["selected"] == sorted(touched) and p["nselected"] == len(touched)
    assert p["sel_bytes"] == sum(rows[m][2] for m in touched)
    return p


def test_rows_are_what_zlib_decodes(mixed):
    blob, data, rows = mixed
    members = gunzip_members(blob)
    starts, end = rm.member_starts(rows)
    assert starts == [s for s, _ in members] and end == len(blob)
    assert [r[2] for r in rows] == [len(d) for _, d in members] and b"".join(d for _, d in members) == data
    assert rm.total_of(rows) == len(data)


def test_byte_ranges_against_slices(mixed):
    _, data, rows = mixed
    rng = np.random.default_rng(1)
    total = len(data)
    begins = [int(x) for x in rng.integers(0, total, 60)]
    ends = [min(total, b + int(x)) for b, x in zip(begins, rng.integers(0, 900, 60))]
    for r in rows:                                                       # every member exactly, and shifted by one at both ends
        for db, de in ((0, 0), (-1, 1), (1, -1), (1, 1), (-1, -1)):
            b, e = r[3] + db, r[3] + r[2] + de
            if 0 <= b <= e:
                begins.append(b)
                ends.append(e)
    begins += [0, total, total - 1, 0]
    ends += [total, total, total, 0]
    check_against_slices(rows, data, rm.BYTES, begins, ends, [(b, min(e, total)) for b, e in zip(begins, ends)])


def test_byte_range_rules_one_case_each(mixed):
    _, data, rows = mixed
    total = len(data)
    cases = [
        (10, 9, None),                                   # begin > end: refused
        (10, total + 1000, (10, total)),                 # end is clipped to the total
        (total, total + 5, (total, total)),              # begin == total: no bytes, accepted
        (total + 7, total + 9, (total, total)),          # begin past the total: no bytes, accepted
        (total + 9, total + 7, None),                    # ... but begin > end is refused wherever it lies
        (33, 33, (33, 33)),                              # an empty range
        (0, 1 << 63, (0, total)),                        # clipped first, so not "too long"
    ]
    p = check_against_slices(rows, data, rm.BYTES, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert p["q_status"] == [1, 0, 0, 0, 1, 0, 0]
    # a range ending on a member's last byte does not select the next member; empty members are never selected
    r = rows[4]
    p = rm.plan(rows, rm.BYTES, [r[3]], [r[3] + r[2]])
    assert p["selected"] == [4]
    p = rm.plan(rows, rm.BYTES, [r[3] + r[2] - 1], [r[3] + r[2] + 1])    # across the empty members 5 and 6
    assert p["selected"] == [4, 7]
    p = rm.plan(rows, rm.BYTES, [0], [total])
    assert p["selected"] == [m for m in range(24) if m not in (5, 6, 13)] and p["sel_bytes"] == total


def test_ranges_of_four_gib_are_refused_with_status_two():
    rows = [(18, 30, 100, 0, 0), (66, 30, 0xffffffff, 100, 0), (114, 30, 0xffffffff, 100 + 0xffffffff, 0),
            (162, 30, 50, 100 + 2 * 0xffffffff, 0)]
    total = rm.total_of(rows)
    p = rm.plan(rows, rm.BYTES, [0, 0, 1, total - 50, 5], [1 << 32, (1 << 32) - 1, (1 << 32) + 1, total, total])
    assert p["q_status"] == [2, 0, 2, 0, 2] and p["q_len"] == [0, (1 << 32) - 1, 0, 50, 0]
    assert p["selected"] == [0, 1, 3] and p["nrefused"] == 3


def test_virtual_offsets_against_slices(mixed):
    blob, data, rows = mixed
    starts, end = rm.member_starts(rows)
    total = len(data)
    V = rm.voffset
    begins, ends, want = [], [], []

    def case(b, e, span):
        begins.append(b)
        ends.append(e)
        want.append(span)
    for m, r in enumerate(rows):
        s, off, size = starts[m], r[3], r[2]
        case(V(s, 0), V(s, size), (off, off + size))                     # the whole member
        case(V(s, size), V(s, size), (off + size, off + size))           # uoffset == ISIZE is valid
        case(V(s, 0), V(s, size + 1), None)                              # uoffset past ISIZE
        case(V(s + 1, 0), V(s, size), None)                              # coffset inside the header
        case(V(r[0], 0), V(s, size), None)                               # coffset of the payload
        case(V(s, 0), V(end, 0), (off, total))                           # to the end of the file
        if m + 1 < len(rows):
            case(V(s, size // 2), V(starts[m + 1], 0), (off + size // 2, off + size))
        if size:
            case(V(s, size), V(s, 0), None)                              # U(begin) > U(end)
    case(V(end, 0), V(end, 0), (total, total))                           # end of file, uoffset 0: the total
    case(V(0, 0), V(end, 1), None)                                       # end of file, uoffset 1
    case(V(end + 1, 0), V(end + 1, 0), None)
    case(V(0, 0), V(starts[9], 3), (0, rows[9][3] + 3))
    check_against_slices(rows, data, rm.VOFFSET, begins, ends, want)
    # the same position named through an empty member or through its neighbour
    assert rm.position(rows, V(starts[5], 0)) == rm.position(rows, V(starts[6], 0)) == rm.position(rows, V(starts[7], 0))
    assert rm.position(rows, V(starts[5], 1)) is None


def test_overlapping_nested_duplicate_unsorted(mixed):
    _, data, rows = mixed
    begins = [500, 100, 100, 150, 90, 2000, 0]
    ends = [900, 400, 400, 200, 120, 2500, 50]
    p = check_against_slices(rows, data, rm.BYTES, begins, ends, list(zip(begins, ends)))
    assert p["out_bytes"] == sum(e - b for b, e in zip(begins, ends))
