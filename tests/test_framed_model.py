"""The model of the framed inflate and the size pass (tests/framed_model.py) against the reference's own functions --
libdeflate_deflate_decompress_ex, libdeflate_zlib_decompress_ex, libdeflate_gzip_decompress_ex of oracle/_ref/libref.so --
and against zlib, on every member of tests/framed_gen.py.  CPU only."""
import ctypes
import zlib

import numpy as np
import pytest

import framed_gen
import framed_model as M
import hdtest

REF_FN = {M.RAW: "libdeflate_deflate_decompress_ex", M.ZLIB: "libdeflate_zlib_decompress_ex",
          M.GZIP: "libdeflate_gzip_decompress_ex"}
WBITS = {M.RAW: -15, M.ZLIB: 15, M.GZIP: 31}


@pytest.fixture(scope="module")
def members():
    return framed_gen.members()


@pytest.fixture(scope="module")
def sizes(members):
    """the size pass's answer for every member, once"""
    return [M.size(m.data, m.frame) for m in members]


def test_generator_covers_the_header_and_trailer_shapes(members, sizes):
    names = {m.name for m in members}
    for want in ("gzip/combo15_x65535_n300", "gzip/combo0_x0_n0", "gzip/name70000", "gzip/tiny17", "gzip/tiny18", "zlib/tiny5",
                 "zlib/tiny6", "gzip/name_leaves_7", "gzip/name_leaves_8", "gzip/hcrc_leaves_7", "gzip/extra_leaves_8",
                 "zlib/cinfo8", "zlib/fdict", "zlib/fcheck_plus1", "zlib/cm7", "gzip/crc_bit31", "gzip/isize_bit0",
                 "zlib/adler_bit17", "gzip/trailer_cut1", "gzip/garbage100", "gzip/pair", "zlib/pair", "raw/pair",
                 "gzip/reserved_20", "gzip/reserved_40", "gzip/reserved_80", "gzip/bad_id1", "gzip/bad_id2", "gzip/bad_cm",
                 "gzip/name_no_nul_at_all"):
        assert want in names, want
    # all sixteen flag combinations, and the payload at every offset mod 4, among the members that decode
    combos, mod4 = set(), set()
    for m, (st, _, _) in zip(members, sizes):
        if m.frame == M.GZIP and st == 0:
            combos.add((m.data[3] >> 1) & 15)
            mod4.add(M.open_member(m.data, M.GZIP) % 4)
    assert combos == set(range(16)) and mod4 == {0, 1, 2, 3}
    # members built to be valid are, with the size they were built from
    for m, (st, sz, used) in zip(members, sizes):
        if m.plain is not None:
            assert (st, sz) == (0, len(m.plain)), m.name
            assert 0 < used <= len(m.data), m.name
    assert sum(1 for s in sizes if s[0] == 0) > 1500 and sum(1 for s in sizes if s[0] == 1) > 400


def test_size_pass_is_the_framed_verdict_without_the_check_value(members, sizes):
    """status 0 from the size pass: the framed call with exactly that room fails on the check value or not at all; one byte
    less is status 3 before any check; every other status is the framed call's in ample room"""
    for m, (st, sz, used) in zip(members, sizes):
        f = M.framed(m.data, m.frame, sz if st == 0 else 1 << 21)
        if st == 0:
            assert f[0] in (0, 1), m.name
            if f[0] == 0:
                assert f[1:3] == (sz, used), m.name
            else:
                assert "_bit" in m.name or m.plain is None, m.name       # only a wrong check value is left
            if sz:
                assert M.framed(m.data, m.frame, sz - 1)[0] == 3, m.name
        else:
            assert f[0] == st, m.name


def test_model_against_the_reference_functions(members, sizes):
    ref = hdtest.ref()
    if ref is None:
        pytest.skip("oracle/_ref/libref.so not built")
    ref.libdeflate_alloc_decompressor.restype = ctypes.c_void_p
    d = ctypes.c_void_p(ref.libdeflate_alloc_decompressor())
    checked = 0
    for m, (st, sz, used) in zip(members, sizes):
        fn = getattr(ref, REF_FN[m.frame])
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                       ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
        src = hdtest.as_u8(m.data)
        # ample room, exact room, room - 1 (for a member that does not decode: ample, and two small rooms)
        rooms = [sz + 1000, sz, sz - 1] if st == 0 and sz else [1 << 21, 100, 0]
        for room in rooms:
            dst = np.zeros(max(room, 1), dtype=np.uint8)
            a_in, a_out = ctypes.c_size_t(0), ctypes.c_size_t(0)
            r = fn(d, hdtest._ptr(src), len(src), hdtest._ptr(dst), room, ctypes.byref(a_in), ctypes.byref(a_out))
            f = M.framed(m.data, m.frame, room)
            assert f[0] == r, (m.name, room, f[0], r)
            if r == 0:
                assert (f[1], f[2]) == (a_out.value, a_in.value), (m.name, room)
                assert f[4] == dst[:a_out.value].tobytes(), (m.name, room)
            checked += 1
        # the size pass: the reference in ample room, but for a wrong CRC-32 / Adler-32
        dst = np.zeros(max(sz, 1 << 21), dtype=np.uint8)
        a_in, a_out = ctypes.c_size_t(0), ctypes.c_size_t(0)
        r = fn(d, hdtest._ptr(src), len(src), hdtest._ptr(dst), len(dst), ctypes.byref(a_in), ctypes.byref(a_out))
        if r == 0:
            assert (st, sz, used) == (0, a_out.value, a_in.value), m.name
        elif st == 0:
            assert r == 1 and ("crc_bit" in m.name or "adler_bit" in m.name or m.plain is None), m.name
        else:
            assert st == r, m.name
    ref.libdeflate_free_decompressor.argtypes = [ctypes.c_void_p]
    ref.libdeflate_free_decompressor(d)
    assert checked > 7000


def test_model_against_zlib_on_valid_members(members):
    n = 0
    for m in members:
        if m.plain is None or not m.zlib:
            continue
        o = zlib.decompressobj(WBITS[m.frame])
        out = o.decompress(m.data)
        assert o.eof and out == m.plain, m.name
        st, olen, used, check, data = M.framed(m.data, m.frame, len(m.plain))
        assert (st, olen, data) == (0, len(m.plain), m.plain), m.name
        assert used == len(m.data) - len(o.unused_data), m.name
        assert check == (zlib.adler32(out) if m.frame == M.ZLIB else zlib.crc32(out)), m.name
        n += 1
    assert n > 1500
