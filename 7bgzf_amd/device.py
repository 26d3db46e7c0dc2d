"""Device-resident view of the batch API for bench.py and the GPU tests: torch
tensors own the HBM buffers (torch is plumbing here -- allocation, streams,
torch.distributed), libhipdeflate.so does the work on the current stream."""
import ctypes
import importlib

import numpy as np
import torch

_pkg = importlib.import_module(__package__)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class DeviceDeflate:
    """Pre-allocated buffers for compressing `nblocks` blocks that live in HBM."""

    def __init__(self, nblocks, slot=65536, device="cuda"):
        self.nblocks = nblocks
        self.slot = slot
        self.slots = torch.empty(nblocks * slot, dtype=torch.uint8, device=device)
        self.out_len = torch.zeros(nblocks, dtype=torch.int32, device=device)
        self.crc = torch.zeros(nblocks, dtype=torch.int32, device=device)
        self.status = torch.zeros(nblocks, dtype=torch.int32, device=device)
        self.dst_off = torch.zeros(nblocks, dtype=torch.int64, device=device)
        self.total = torch.zeros(1, dtype=torch.int64, device=device)

    def run(self, data, in_off, in_len, level=1, frame=_pkg.FRAME_BGZF):
        rc = _pkg.lib().hipdeflate_batch_deflate_dev(
            _ptr(data), _ptr(in_off), _ptr(in_len), self.nblocks, level, frame, _ptr(self.slots), self.slot,
            self.slot, _ptr(self.out_len), _ptr(self.crc), _ptr(self.status), _stream())
        _pkg._check(rc, "hipdeflate_batch_deflate_dev")

    def scan(self, base=0):
        rc = _pkg.lib().hipdeflate_scan_sizes_dev(_ptr(self.out_len), self.nblocks, base, _ptr(self.dst_off),
                                                  _ptr(self.total), _stream())
        _pkg._check(rc, "hipdeflate_scan_sizes_dev")

    def compact(self, dst, span_base=0):
        """members -> dst; with span_base != 0 dst is this rank's span of a sharded stream and
        dst_off[] (scan(base=span_base)) are offsets in the whole stream"""
        rc = _pkg.lib().hipdeflate_compact_span_dev(_ptr(self.slots), self.slot, _ptr(self.out_len),
                                                    _ptr(self.dst_off), self.nblocks, _ptr(dst), span_base, _stream())
        _pkg._check(rc, "hipdeflate_compact_span_dev")


class DeviceInflate:
    """Decode a container file (BGZF, MiGz, any stream of the member kinds hd7bgzf -d reads) that lives in HBM: the
    member table is made on the device (hipdeflate_index_members_dev), so no byte of the file visits the host.  Owns the
    five table tensors of `max_members` entries plus out_len / crc / status of the inflate."""

    def __init__(self, max_members, device="cuda"):
        self.max_members = max_members

        def table(dtype):
            return torch.zeros(max_members, dtype=dtype, device=device)
        self.in_off, self.out_off = table(torch.int64), table(torch.int64)
        self.in_len, self.out_size, self.crc_want = table(torch.int32), table(torch.int32), table(torch.int32)
        self.out_len, self.crc, self.status = table(torch.int32), table(torch.int32), table(torch.int32)
        self.nmembers = None             # entries the last index() filled

    def index(self, blob):
        """blob: uint8 tensor, 16-byte aligned -> MemberSummary; the tables hold min(nmembers, max_members) entries"""
        summary = _pkg.MemberSummary()
        rc = _pkg.lib().hipdeflate_index_members_dev(
            _ptr(blob), blob.numel(), self.max_members, _ptr(self.in_off), _ptr(self.in_len), _ptr(self.out_size),
            _ptr(self.out_off), _ptr(self.crc_want), ctypes.byref(summary), _stream())
        _pkg._check(rc, "hipdeflate_index_members_dev")
        self.nmembers = min(summary.nmembers, self.max_members)
        return summary

    def index_any(self, blob, first_offset=0, max_member_in=0):
        """index() for members that may state no length (hipdeflate_index_members_any_dev): the walk starts at first_offset, a
        member without a known length field is sized by decoding at most max_member_in of its bytes (0: no bound below the
        library's) -> MemberAnySummary; the same tensors are filled, so run(blob, out, summary) and read_ranges work on them"""
        summary = _pkg.MemberAnySummary()
        rc = _pkg.lib().hipdeflate_index_members_any_dev(
            _ptr(blob), blob.numel(), first_offset, self.max_members, max_member_in, _ptr(self.in_off), _ptr(self.in_len),
            _ptr(self.out_size), _ptr(self.out_off), _ptr(self.crc_want), ctypes.byref(summary), _stream())
        _pkg._check(rc, "hipdeflate_index_members_any_dev")
        self.nmembers = min(summary.nmembers, self.max_members)
        return summary

    def verify(self, nmembers):
        """-> index of the first member whose inflate result disagrees with its trailer, nmembers if none"""
        first_bad = ctypes.c_uint64()
        rc = _pkg.lib().hipdeflate_verify_members_dev(_ptr(self.status), _ptr(self.out_len), _ptr(self.crc),
                                                      _ptr(self.out_size), _ptr(self.crc_want), nmembers,
                                                      ctypes.byref(first_bad), _stream())
        _pkg._check(rc, "hipdeflate_verify_members_dev")
        return first_bad.value

    def run(self, blob, out, summary=None):
        """index, inflate member i to out[out_off[i]:] with room for its ISIZE, verify -> the summary.
        `summary`: what index(blob) has just answered for these tables, to spare the second pass over the blob"""
        s = summary if summary is not None else self.index(blob)
        if s.status:
            why = {1: "not a member", 2: "member cut off", 3: "more members than max_members = %d" % self.max_members,
                   4: "member longer than max_member_in"}
            raise _pkg.HipDeflateError("member index: %s at offset %d (%d members)" % (why[s.status], s.end_offset, s.nmembers))
        if out.numel() < s.out_bytes:
            raise _pkg.HipDeflateError("output of %d bytes, the members hold %d" % (out.numel(), s.out_bytes))
        n = s.nmembers
        if n == 0:
            return s
        device_inflate(blob, self.in_off[:n], self.in_len, out, self.out_off, self.out_size, self.out_len, self.crc, self.status)
        bad = self.verify(n)
        if bad != n:
            raise _pkg.HipDeflateError("member %d: inflate status %d, or CRC32/ISIZE mismatch" % (bad, int(self.status[bad])))
        return s

    def ranges_call(self, blob, begins, ends, kind, nmembers, dst, dst_cap):
        """one hipdeflate_read_ranges_dev on these tables: begins / ends int64 device tensors (the bits of the u64 values),
        dst a uint8 tensor of any alignment or None -> (dst_off, q_len, q_status, RangeSummary)"""
        nq = begins.numel()
        dst_off = torch.zeros(nq, dtype=torch.int64, device=blob.device)
        q_len = torch.zeros(nq, dtype=torch.int32, device=blob.device)
        q_status = torch.zeros(nq, dtype=torch.int32, device=blob.device)
        summary = _pkg.RangeSummary()
        rc = _pkg.lib().hipdeflate_read_ranges_dev(
            _ptr(blob), _ptr(self.in_off), _ptr(self.in_len), _ptr(self.out_size), _ptr(self.out_off), _ptr(self.crc_want),
            nmembers, kind, _ptr(begins), _ptr(ends), nq, _ptr(dst), dst_cap, _ptr(dst_off), _ptr(q_len), _ptr(q_status),
            ctypes.byref(summary), _stream())
        _pkg._check(rc, "hipdeflate_read_ranges_dev")
        return dst_off, q_len, q_status, summary

    def read_ranges(self, blob, begins, ends, kind=_pkg.RANGE_BYTES, nmembers=None):
        """the bytes of the ranges [begins[q], ends[q]) of the decoded file -- offsets in it, or virtual offsets with
        kind=RANGE_VOFFSET -- on the tables index(blob) filled; only the members the ranges touch are inflated.
        -> (out, dst_off, q_len, q_status, RangeSummary): query q is out[dst_off[q]:dst_off[q] + q_len[q]], q_status[q] != 0
        where it was refused (1: no such range, 2: 4 GiB or more)"""
        n = (self.nmembers if self.nmembers is not None else self.max_members) if nmembers is None else nmembers
        begins, ends = _u64_tensor(begins, blob.device), _u64_tensor(ends, blob.device)
        if begins.numel() != ends.numel():
            raise ValueError("%d begins, %d ends" % (begins.numel(), ends.numel()))
        s = self.ranges_call(blob, begins, ends, kind, n, None, 0)[3]             # the sizing call
        out = torch.empty(s.out_bytes, dtype=torch.uint8, device=blob.device)
        dst_off, q_len, q_status, s = self.ranges_call(blob, begins, ends, kind, n, out, out.numel())
        if s.status == 2:
            raise _pkg.HipDeflateError("member %d: inflate status, or CRC32/ISIZE mismatch" % s.bad_member)
        if s.status:
            raise _pkg.HipDeflateError("ranged read: status %d" % s.status)
        return out, dst_off, q_len, q_status, s


def _u64_tensor(v, device):
    """u64 values (a sequence of ints, a numpy array, or an int64 tensor holding their bits) -> int64 device tensor"""
    if isinstance(v, torch.Tensor):
        return v.to(device=device, dtype=torch.int64).contiguous()
    a = np.array([int(x) for x in v], dtype=np.uint64) if not isinstance(v, np.ndarray) else v.astype(np.uint64)
    return torch.from_numpy(a.view(np.int64).copy()).to(device)


def inflate_container(blob):
    """uint8 tensor holding a whole container file -> uint8 tensor of its contents; nothing visits the host.
    Two passes over the blob: a table of no entries answers status 3 and the number of members the stream has, the
    table of that size then gives out_bytes and is the one the inflate runs on."""
    d = DeviceInflate(DeviceInflate(0, blob.device).index(blob).nmembers, blob.device)
    s = d.index(blob)
    out = torch.empty(s.out_bytes, dtype=torch.uint8, device=blob.device)
    d.run(blob, out, s)
    return out


def _index_any_sized(blob, first_offset, max_member_in):
    """the sizing call, then the index on tables of that size -> (DeviceInflate, MemberAnySummary)"""
    n = DeviceInflate(0, blob.device).index_any(blob, first_offset, max_member_in).nmembers
    d = DeviceInflate(n, blob.device)
    return d, d.index_any(blob, first_offset, max_member_in)


def inflate_gzip_members(blob, max_member_in=0):
    """uint8 tensor, 16-byte aligned, holding a file of gzip members with or without a length field (`cat a.gz b.gz`, the
    records of a .warc.gz) -> uint8 tensor of its contents: the sizing call, the index, one allocation, the batch inflate
    and the verify, like inflate_container.  A member longer than max_member_in (0: HD_INFLATE_MAX_IN - 1) raises."""
    d, s = _index_any_sized(blob, 0, max_member_in)
    out = torch.empty(s.out_bytes, dtype=torch.uint8, device=blob.device)
    d.run(blob, out, s)
    return out


def inflate_gzip_file(blob, max_member_in=0):
    """inflate_gzip_members for any .gz at all: where the index stops at a member longer than max_member_in (status 4), that
    one member is decoded as a plain stream in parallel rows (inflate_stream_blocks, on a 16-byte aligned copy of the blob
    from the member on) and the index resumes behind it -> uint8 tensor of the file's contents"""
    parts, at, n = [], 0, blob.numel()
    while at < n:
        d, s = _index_any_sized(blob, at, max_member_in)
        if s.status not in (0, 4):
            why = {1: "not a member", 2: "member cut off"}
            raise _pkg.HipDeflateError("member index: %s at offset %d (%d members)" % (why.get(s.status, "?"), s.end_offset, s.nmembers))
        if s.nmembers:
            out = torch.empty(s.out_bytes, dtype=torch.uint8, device=blob.device)
            s4, s.status = s.status, 0
            d.run(blob, out, s)
            s.status = s4
            parts.append(out)
        at = s.end_offset
        if s.status == 4:
            tail = torch.empty(n - at + 16, dtype=torch.uint8, device=blob.device)[:n - at]       # (a fresh allocation: aligned)
            tail.copy_(blob[at:])
            out, x = inflate_stream_blocks(tail, _pkg.FRAME_GZIP)
            parts.append(out)
            at += x.end_offset
    return torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device=blob.device)


def read_ranges(blob, begins, ends, kind=_pkg.RANGE_BYTES):
    """uint8 tensor holding a whole container file + ranges of its contents -> what DeviceInflate.read_ranges answers;
    the file is indexed first, as inflate_container does"""
    d = DeviceInflate(DeviceInflate(0, blob.device).index(blob).nmembers, blob.device)
    s = d.index(blob)
    if s.status:
        why = {1: "not a member", 2: "member cut off"}
        raise _pkg.HipDeflateError("member index: %s at offset %d (%d members)" % (why[s.status], s.end_offset, s.nmembers))
    return d.read_ranges(blob, begins, ends, kind)


def deflate_stream_call(data, level, frame, chunk, dst, dst_cap, chunk_off):
    """one hipdeflate_stream_deflate_dev: data a 16-byte aligned uint8 tensor, dst a 16-byte aligned uint8 tensor or None,
    chunk_off an int64 tensor of nchunks + 1 entries or None -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_deflate_dev(_ptr(data), data.numel(), chunk, level, frame, _ptr(dst), dst_cap,
                                                  _ptr(chunk_off), ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_deflate_dev")
    return summary


def _deflate_stream(call, data, level, frame, chunk):
    n = data.numel()
    nchunks = (n + chunk - 1) // chunk
    bound = int(_pkg.lib().hipdeflate_stream_bound(n, chunk, level, frame))
    if bound == 0:
        raise ValueError("chunk = %d: a multiple of 16 in [16, 64 MiB]" % chunk)
    dst = torch.empty(bound, dtype=torch.uint8, device=data.device)
    chunk_off = torch.zeros(nchunks + 1, dtype=torch.int64, device=data.device)
    s = call(data, level, frame, chunk, dst, bound, chunk_off)
    if s.status:
        raise _pkg.HipDeflateError("stream encode: status %d, chunk %d" % (s.status, s.bad_chunk))
    return dst[:s.out_bytes], chunk_off, s


def deflate_stream(data, level=6, frame=_pkg.FRAME_GZIP, chunk=1 << 16):
    """uint8 tensor -> (stream, chunk_off, StreamSummary): ONE raw / zlib / gzip stream of the whole tensor, coded in
    independent chunks of `chunk` bytes side by side.  The stream is allocated at hipdeflate_stream_bound and narrowed to
    out_bytes; chunk_off (int64, nchunks + 1 entries) is the table inflate_stream wants."""
    return _deflate_stream(deflate_stream_call, data, level, frame, chunk)


def deflate_stream_carry_call(data, level, frame, chunk, dst, dst_cap, chunk_off):
    """one hipdeflate_stream_deflate_carry_dev: deflate_stream_call's arguments -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_deflate_carry_dev(_ptr(data), data.numel(), chunk, level, frame, _ptr(dst), dst_cap,
                                                        _ptr(chunk_off), ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_deflate_carry_dev")
    return summary


def deflate_stream_carry(data, level=6, frame=_pkg.FRAME_GZIP, chunk=1 << 16):
    """deflate_stream with every chunk primed by the min(32768, its offset) & ~1023 bytes in front of it (levels 3..9): the
    one-block ratio at any chunk size, for streams that serial inflaters read.  -> (stream, chunk_off, StreamSummary);
    the decode on the device is inflate_stream_carry, not inflate_stream."""
    return _deflate_stream(deflate_stream_carry_call, data, level, frame, chunk)


def inflate_stream_call(stream, frame, chunk_off, nchunks, chunk, out_bytes, out, out_cap):
    """one hipdeflate_stream_inflate_dev -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_inflate_dev(_ptr(stream), stream.numel(), frame, _ptr(chunk_off), nchunks, chunk,
                                                  out_bytes, _ptr(out), out_cap, ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_inflate_dev")
    return summary


def inflate_stream(stream, chunk_off, chunk, out_bytes, frame=_pkg.FRAME_GZIP):
    """the inverse of deflate_stream: stream a 16-byte aligned uint8 tensor, chunk_off its table (int64 tensor or a
    sequence of ints, nchunks + 1 entries) -> uint8 tensor of out_bytes; the chunks are inflated side by side and the
    result is held to the trailer"""
    chunk_off = _u64_tensor(chunk_off, stream.device)
    out = torch.empty(out_bytes, dtype=torch.uint8, device=stream.device)
    s = inflate_stream_call(stream, frame, chunk_off, chunk_off.numel() - 1, chunk, out_bytes, out, out_bytes)
    if s.status:
        why = {1: "not such a stream, or a bad table", 2: "a chunk or the check disagrees", 3: "room too small"}
        raise _pkg.HipDeflateError("stream decode: %s (status %d, bad_chunk %d of %d)" % (why.get(s.status, "?"), s.status,
                                                                                         s.bad_chunk, s.nchunks))
    return out


def index_stream_call(stream, frame, max_chunks, max_chunk_in, in_off, in_len, out_size, out_off):
    """one hipdeflate_stream_index_dev: stream a 16-byte aligned uint8 tensor, the four tables int64 / int32 tensors of
    max_chunks entries (None with max_chunks == 0: the sizing call) -> StreamIndexSummary"""
    summary = _pkg.StreamIndexSummary()
    rc = _pkg.lib().hipdeflate_stream_index_dev(_ptr(stream), stream.numel(), frame, max_chunks, max_chunk_in, _ptr(in_off),
                                                _ptr(in_len), _ptr(out_size), _ptr(out_off), ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_index_dev")
    return summary


def index_stream(stream, frame=_pkg.FRAME_GZIP, max_chunks=None, max_chunk_in=0):
    """the chunk table of a stream in flush form whose table nobody kept -> (in_off, in_len, out_size, out_off,
    StreamIndexSummary): device tensors of max_chunks entries, of which min(nchunks, max_chunks) are filled.  Without
    max_chunks the tables get one row per 64 stream bytes, and where a stream has more (status 3 names the number) it is
    indexed again on tables of that size."""
    dev = stream.device

    def run(n):
        t = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev))
        return t + (index_stream_call(stream, frame, n, max_chunk_in, *t),)

    if max_chunks is not None:
        return run(max_chunks)
    r = run(stream.numel() // 64 + 16)
    return run(r[4].nchunks) if r[4].status == 3 else r


def inflate_stream_table_call(stream, frame, in_off, in_len, out_size, out_off, nchunks, out, out_cap):
    """one hipdeflate_stream_inflate_table_dev -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_inflate_table_dev(_ptr(stream), stream.numel(), frame, _ptr(in_off), _ptr(in_len),
                                                        _ptr(out_size), _ptr(out_off), nchunks, _ptr(out), out_cap,
                                                        ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_inflate_table_dev")
    return summary


def inflate_stream_auto(stream, frame=_pkg.FRAME_GZIP):
    """a raw / zlib / gzip stream in flush form, 16-byte aligned uint8 tensor -> (uint8 tensor of its contents,
    StreamIndexSummary): index, one allocation, the chunks inflated side by side and held to the trailer.  Only the two
    summaries visit the host.  Bytes behind the trailer are left alone: summary.end_offset says where they start."""
    in_off, in_len, out_size, out_off, x = index_stream(stream, frame)
    if x.status:
        why = {1: "a piece does not decode, or the header is refused", 2: "the stream is cut"}
        raise _pkg.HipDeflateError("stream index: %s at offset %d (status %d, %d chunks)" % (why.get(x.status, "?"), x.end_offset,
                                                                                            x.status, x.nchunks))
    out = torch.empty(x.out_bytes, dtype=torch.uint8, device=stream.device)
    s = inflate_stream_table_call(stream, frame, in_off, in_len, out_size, out_off, x.nchunks, out, x.out_bytes)
    if s.status:
        why = {1: "a bad table", 2: "a chunk or the check disagrees", 3: "room too small"}
        raise _pkg.HipDeflateError("stream decode: %s (status %d, bad_chunk %d of %d)" % (why.get(s.status, "?"), s.status,
                                                                                         s.bad_chunk, s.nchunks))
    return out, x


def index_stream_carry_call(stream, frame, max_chunks, max_chunk_in, in_off, in_len, out_size, out_off, reach):
    """one hipdeflate_stream_index_carry_dev: index_stream_call with the reach table (int32 tensor of max_chunks entries)
    -> StreamIndexSummary"""
    summary = _pkg.StreamIndexSummary()
    rc = _pkg.lib().hipdeflate_stream_index_carry_dev(_ptr(stream), stream.numel(), frame, max_chunks, max_chunk_in, _ptr(in_off),
                                                      _ptr(in_len), _ptr(out_size), _ptr(out_off), _ptr(reach),
                                                      ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_index_carry_dev")
    return summary


def index_stream_carry(stream, frame=_pkg.FRAME_GZIP, max_chunks=None, max_chunk_in=0):
    """index_stream for a stream whose flushes carry the window -> (in_off, in_len, out_size, out_off, reach,
    StreamIndexSummary); indexed again on tables of the stream's size where the first ones are too small (status 3)"""
    dev = stream.device

    def run(n):
        t = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev))
        return t + (index_stream_carry_call(stream, frame, n, max_chunk_in, *t),)

    if max_chunks is not None:
        return run(max_chunks)
    r = run(stream.numel() // 64 + 16)
    return run(r[5].nchunks) if r[5].status == 3 else r


def inflate_stream_carry_call(stream, frame, in_off, in_len, out_size, out_off, reach, nchunks, out, out_cap):
    """one hipdeflate_stream_inflate_carry_dev -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_inflate_carry_dev(_ptr(stream), stream.numel(), frame, _ptr(in_off), _ptr(in_len),
                                                        _ptr(out_size), _ptr(out_off), _ptr(reach), nchunks, _ptr(out), out_cap,
                                                        ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_inflate_carry_dev")
    return summary


def inflate_stream_carry(stream, frame=_pkg.FRAME_GZIP):
    """inflate_stream_auto for a stream whose flushes carry the window (pigz, zlib's Z_SYNC_FLUSH) -> (uint8 tensor of its
    contents, StreamIndexSummary): the carry index, one allocation, the rows decoded side by side and held to the trailer"""
    in_off, in_len, out_size, out_off, reach, x = index_stream_carry(stream, frame)
    if x.status:
        why = {1: "a piece does not decode, or the header is refused", 2: "the stream is cut"}
        raise _pkg.HipDeflateError("stream index: %s at offset %d (status %d, %d chunks)" % (why.get(x.status, "?"), x.end_offset,
                                                                                            x.status, x.nchunks))
    out = torch.empty(x.out_bytes, dtype=torch.uint8, device=stream.device)
    s = inflate_stream_carry_call(stream, frame, in_off, in_len, out_size, out_off, reach, x.nchunks, out, x.out_bytes)
    if s.status:
        why = {1: "a bad table", 2: "a chunk or the check disagrees", 3: "room too small"}
        raise _pkg.HipDeflateError("stream decode: %s (status %d, bad_chunk %d of %d)" % (why.get(s.status, "?"), s.status,
                                                                                         s.bad_chunk, s.nchunks))
    return out, x


def index_stream_blocks_call(stream, frame, max_rows, max_chunk_in, row_bytes, in_off, in_len, out_size, out_off, reach):
    """one hipdeflate_stream_index_blocks_dev: stream a 16-byte aligned uint8 tensor, the five tables int64 / int32 tensors of
    max_rows entries (None with max_rows == 0: the sizing call), in_off and in_len in BITS -> BlockIndexSummary"""
    summary = _pkg.BlockIndexSummary()
    rc = _pkg.lib().hipdeflate_stream_index_blocks_dev(_ptr(stream), stream.numel(), frame, max_rows, max_chunk_in, row_bytes,
                                                       _ptr(in_off), _ptr(in_len), _ptr(out_size), _ptr(out_off), _ptr(reach),
                                                       ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_index_blocks_dev")
    return summary


def index_stream_blocks(stream, frame=_pkg.FRAME_GZIP, max_rows=None, max_chunk_in=0, row_bytes=0):
    """the row table of a plain stream, which has no flush point: its blocks found at their bits and merged into rows of
    about row_bytes of output (0: BLOCK_ROW_BYTES) -> (in_off, in_len, out_size, out_off, reach, BlockIndexSummary), in_off
    and in_len in BITS.  Without max_rows the tables get one row per 64 stream bytes, and where a chain has more (status 3
    names the number) the stream is indexed again on tables of that size."""
    dev = stream.device

    def run(n):
        t = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev))
        return t + (index_stream_blocks_call(stream, frame, n, max_chunk_in, row_bytes, *t),)

    if max_rows is not None:
        return run(max_rows)
    r = run(stream.numel() // 64 + 16)
    return run(r[5].nrows) if r[5].status == 3 else r


def inflate_stream_blocks_call(stream, frame, in_off, in_len, out_size, out_off, reach, nrows, out, out_cap):
    """one hipdeflate_stream_inflate_blocks_dev -> StreamSummary"""
    summary = _pkg.StreamSummary()
    rc = _pkg.lib().hipdeflate_stream_inflate_blocks_dev(_ptr(stream), stream.numel(), frame, _ptr(in_off), _ptr(in_len),
                                                         _ptr(out_size), _ptr(out_off), _ptr(reach), nrows, _ptr(out), out_cap,
                                                         ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_inflate_blocks_dev")
    return summary


def inflate_stream_blocks(stream, frame=_pkg.FRAME_GZIP):
    """inflate_stream_auto for a plain stream, which has no flush point (gzip, zlib.compress, an IDAT) -> (uint8 tensor of
    its contents, BlockIndexSummary): the block index, one allocation, the rows decoded side by side and held to the trailer.
    The index runs with max_chunk_in = BLOCK_PIECE_IN first, which bounds what a false candidate costs, and unbounded only
    where that answers status 1."""
    in_off, in_len, out_size, out_off, reach, x = index_stream_blocks(stream, frame, max_chunk_in=_pkg.BLOCK_PIECE_IN)
    if x.status == 1 and stream.numel() > _pkg.BLOCK_PIECE_IN:
        in_off, in_len, out_size, out_off, reach, x = index_stream_blocks(stream, frame)
    if x.status:
        why = {1: "a piece does not decode, or the header is refused", 2: "the stream is cut"}
        raise _pkg.HipDeflateError("block index: %s at bit %d (status %d, %d rows)" % (why.get(x.status, "?"), x.end_bit, x.status,
                                                                                       x.nrows))
    out = torch.empty(x.out_bytes, dtype=torch.uint8, device=stream.device)
    s = inflate_stream_blocks_call(stream, frame, in_off, in_len, out_size, out_off, reach, x.nrows, out, x.out_bytes)
    if s.status:
        why = {1: "a bad table", 2: "a row or the check disagrees", 3: "room too small"}
        raise _pkg.HipDeflateError("stream decode: %s (status %d, bad_chunk %d of %d)" % (why.get(s.status, "?"), s.status,
                                                                                         s.bad_chunk, s.nchunks))
    return out, x


def stream_windows_call(out, out_size, out_off, reach, nrows, win_off, win, win_cap, row_check):
    """one hipdeflate_stream_windows_dev: out the decoded stream, the three columns of its row table, win_off an int64
    tensor of nrows + 1 entries, win a uint8 tensor or None (the sizing call), row_check an int32 tensor -> WindowSummary"""
    summary = _pkg.WindowSummary()
    rc = _pkg.lib().hipdeflate_stream_windows_dev(_ptr(out), out.numel(), _ptr(out_size), _ptr(out_off), _ptr(reach), nrows,
                                                  _ptr(win_off), _ptr(win), win_cap, _ptr(row_check), ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_windows_dev")
    return summary


def stream_read_ranges_call(stream, frame, unit, in_off, in_len, out_size, out_off, reach, win_off, win, win_bytes, row_check, nrows,
                            begins, ends, dst, dst_cap):
    """one hipdeflate_stream_read_ranges_dev: begins / ends int64 device tensors (the bits of the u64 values), dst a uint8
    tensor of any alignment or None, row_check an int32 tensor or None -> (dst_off, q_len, q_status, RangeSummary)"""
    nq = begins.numel()
    dst_off = torch.zeros(nq, dtype=torch.int64, device=stream.device)
    q_len = torch.zeros(nq, dtype=torch.int32, device=stream.device)
    q_status = torch.zeros(nq, dtype=torch.int32, device=stream.device)
    summary = _pkg.RangeSummary()
    rc = _pkg.lib().hipdeflate_stream_read_ranges_dev(
        _ptr(stream), stream.numel(), frame, unit, _ptr(in_off), _ptr(in_len), _ptr(out_size), _ptr(out_off), _ptr(reach),
        _ptr(win_off), _ptr(win), win_bytes, _ptr(row_check), nrows, _ptr(begins), _ptr(ends), nq, _ptr(dst), dst_cap,
        _ptr(dst_off), _ptr(q_len), _ptr(q_status), ctypes.byref(summary), _stream())
    _pkg._check(rc, "hipdeflate_stream_read_ranges_dev")
    return dst_off, q_len, q_status, summary


class SeekIndex:
    """A seek index on ONE raw / zlib / gzip stream resident in HBM: its row table (the block index's, in bits, or the carry
    index's, in bytes), the window in front of every row and the CRC-32 of every row's bytes.  build() pays one full decode;
    a read then decodes only the rows it touches.  The windows hold at most 32 KiB a row: row_bytes is what they cost."""

    VERSION = 1
    COLUMNS = ("in_off", "in_len", "out_size", "out_off", "reach", "win_off", "row_check")
    _DTYPES = {"in_off": np.int64, "in_len": np.int32, "out_size": np.int32, "out_off": np.int64, "reach": np.int32,
               "win_off": np.int64, "row_check": np.int32}

    def __init__(self, stream, frame, unit, nbytes, columns, win):
        """stream: the uint8 tensor the index belongs to (None: an index that can be saved, not read); columns: a dict of
        the seven COLUMNS, win: the window bytes -- tensors on the stream's device, or numpy arrays where there is no stream"""
        self.stream, self.frame, self.unit, self.nbytes = stream, int(frame), int(unit), int(nbytes)
        self.columns, self.win = dict(columns), win
        self.nrows = len(self.columns["in_off"])
        if len(self.columns["win_off"]) != self.nrows + 1 or any(len(self.columns[c]) != self.nrows for c in self.COLUMNS if c != "win_off"):
            raise ValueError("seek index: columns of uneven length")

    @classmethod
    def build(cls, stream, frame=_pkg.FRAME_GZIP, kind="blocks", row_bytes=0):
        """index, full decode, the sizing call, the windows call; raises on any non-zero status"""
        if kind == "blocks":
            in_off, in_len, out_size, out_off, reach, x = index_stream_blocks(stream, frame, row_bytes=row_bytes)
            n, unit, decode = x.nrows, _pkg.ROWS_BITS, inflate_stream_blocks_call
        elif kind == "carry":
            in_off, in_len, out_size, out_off, reach, x = index_stream_carry(stream, frame)
            n, unit, decode = x.nchunks, _pkg.ROWS_BYTES, inflate_stream_carry_call
        else:
            raise ValueError("kind = %r: 'blocks' or 'carry'" % (kind,))
        if x.status:
            raise _pkg.HipDeflateError("seek index: the %s index answers status %d (%d rows)" % (kind, x.status, n))
        out = torch.empty(x.out_bytes, dtype=torch.uint8, device=stream.device)
        s = decode(stream, frame, in_off, in_len, out_size, out_off, reach, n, out, x.out_bytes)
        if s.status:
            raise _pkg.HipDeflateError("seek index: the full decode answers status %d (bad_chunk %d of %d)" % (s.status, s.bad_chunk, n))
        cols = [c[:n].contiguous() for c in (in_off, in_len, out_size, out_off, reach)]
        win_off = torch.zeros(n + 1, dtype=torch.int64, device=stream.device)
        row_check = torch.zeros(n, dtype=torch.int32, device=stream.device)
        w = stream_windows_call(out, cols[2], cols[3], cols[4], n, win_off, None, 0, row_check)
        if w.status not in (0, 3):
            raise _pkg.HipDeflateError("seek index: the windows call answers status %d (row %d)" % (w.status, w.bad_row))
        win = torch.empty(w.win_bytes, dtype=torch.uint8, device=stream.device)
        w = stream_windows_call(out, cols[2], cols[3], cols[4], n, win_off, win, win.numel(), row_check)
        if w.status:
            raise _pkg.HipDeflateError("seek index: the windows call answers status %d (row %d)" % (w.status, w.bad_row))
        return cls(stream, frame, unit, stream.numel(), dict(zip(cls.COLUMNS, cols + [win_off, row_check])), win)

    @property
    def total(self):
        """the decoded bytes of the stream (the table's last row is on the host only behind save / load)"""
        o, s = self.columns["out_off"], self.columns["out_size"]
        return int(o[-1]) + (int(s[-1]) & 0xffffffff) if self.nrows else 0

    def _call(self, begins, ends, dst, dst_cap):
        c = self.columns
        return stream_read_ranges_call(self.stream, self.frame, self.unit, c["in_off"], c["in_len"], c["out_size"], c["out_off"],
                                       c["reach"], c["win_off"], self.win, self.win.numel(), c["row_check"], self.nrows, begins, ends,
                                       dst, dst_cap)

    def read_ranges(self, begins, ends):
        """the bytes of the ranges [begins[q], ends[q]) of the decoded stream; only the rows they touch are decoded
        -> (out, dst_off, q_len, q_status, RangeSummary), as DeviceInflate.read_ranges answers"""
        if self.stream is None:
            raise _pkg.HipDeflateError("seek index: loaded without its stream")
        begins, ends = _u64_tensor(begins, self.stream.device), _u64_tensor(ends, self.stream.device)
        if begins.numel() != ends.numel():
            raise ValueError("%d begins, %d ends" % (begins.numel(), ends.numel()))
        s = self._call(begins, ends, None, 0)[3]                                  # the sizing call
        if s.status not in (0, 3):
            raise _pkg.HipDeflateError("seek read: status %d, row %d" % (s.status, s.bad_member))
        out = torch.empty(s.out_bytes, dtype=torch.uint8, device=self.stream.device)
        dst_off, q_len, q_status, s = self._call(begins, ends, out, out.numel())
        if s.status:
            raise _pkg.HipDeflateError("seek read: status %d, row %d" % (s.status, s.bad_member))
        return out, dst_off, q_len, q_status, s

    def read(self, begin, end):
        """the bytes [begin, end) of the decoded stream -> uint8 tensor"""
        out, _, _, q_status, _ = self.read_ranges([begin], [end])
        if int(q_status[0]):
            raise ValueError("seek read: [%d, %d) is refused (q_status %d)" % (begin, end, int(q_status[0])))
        return out

    def save(self, path):
        """one numpy.savez file: a version number, frame, unit, nbytes, the seven columns and the window bytes"""
        def host(a):
            return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        arrays = {c: host(self.columns[c]).astype(self._DTYPES[c], copy=False) for c in self.COLUMNS}
        with open(path, "wb") as f:
            np.savez(f, version=np.int64(self.VERSION), frame=np.int64(self.frame), unit=np.int64(self.unit),
                     nbytes=np.int64(self.nbytes), win=host(self.win).astype(np.uint8, copy=False), **arrays)

    @classmethod
    def load(cls, path, stream):
        """the index save() wrote, for `stream` (a uint8 device tensor: the columns go to its device; or a bytes-like object,
        for which they stay numpy arrays and nothing touches a device).  Refuses another version, and a stream of another length."""
        with np.load(path) as z:
            version = int(z["version"])
            if version != cls.VERSION:
                raise _pkg.HipDeflateError("seek index: version %d, this is version %d" % (version, cls.VERSION))
            nbytes = int(z["nbytes"])
            have = stream.numel() if isinstance(stream, torch.Tensor) else len(stream)
            if nbytes != have:
                raise _pkg.HipDeflateError("seek index: made for a stream of %d bytes, this one has %d" % (nbytes, have))
            cols = {c: z[c].astype(cls._DTYPES[c]) for c in cls.COLUMNS}
            win, frame, unit = z["win"].astype(np.uint8), int(z["frame"]), int(z["unit"])
        if unit not in (_pkg.ROWS_BYTES, _pkg.ROWS_BITS):
            raise _pkg.HipDeflateError("seek index: unit %d" % unit)
        if isinstance(stream, torch.Tensor):
            cols = {c: torch.from_numpy(a).to(stream.device) for c, a in cols.items()}
            return cls(stream, frame, unit, nbytes, cols, torch.from_numpy(win).to(stream.device))
        return cls(None, frame, unit, nbytes, cols, win)


def check_combine(check, lens, kind=_pkg.CHECK_CRC32):
    """the CRC-32 (kind 0) / Adler-32 (kind 1) of a concatenation from the checks and lengths of its parts: int32 device
    tensors holding the bits of the u32 values -> int"""
    result = ctypes.c_uint32()
    rc = _pkg.lib().hipdeflate_check_combine_dev(_ptr(check), _ptr(lens), check.numel(), kind, ctypes.byref(result), _stream())
    _pkg._check(rc, "hipdeflate_check_combine_dev")
    return result.value


def device_inflate(comp, in_off, in_len, out, out_off, out_cap, out_len, crc, status):
    nb = in_off.numel()
    rc = _pkg.lib().hipdeflate_batch_inflate_dev(_ptr(comp), _ptr(in_off), _ptr(in_len), nb, _ptr(out), _ptr(out_off),
                                                 _ptr(out_cap), _ptr(out_len), _ptr(crc), _ptr(status), _stream())
    _pkg._check(rc, "hipdeflate_batch_inflate_dev")


def inflate_size_call(blob, in_off, in_len, frame, out_size, in_used, status):
    """one hipdeflate_batch_inflate_size_dev over device tensors"""
    rc = _pkg.lib().hipdeflate_batch_inflate_size_dev(_ptr(blob), _ptr(in_off), _ptr(in_len), in_off.numel(), frame,
                                                      _ptr(out_size), _ptr(in_used), _ptr(status), _stream())
    _pkg._check(rc, "hipdeflate_batch_inflate_size_dev")


def inflate_framed_call(blob, in_off, in_len, frame, out, out_off, out_cap, out_len, check, in_used, status):
    """one hipdeflate_batch_inflate_framed_dev over device tensors (check, in_used: a tensor or None)"""
    rc = _pkg.lib().hipdeflate_batch_inflate_framed_dev(_ptr(blob), _ptr(in_off), _ptr(in_len), in_off.numel(), frame, _ptr(out),
                                                        _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(check), _ptr(in_used),
                                                        _ptr(status), _stream())
    _pkg._check(rc, "hipdeflate_batch_inflate_framed_dev")


def inflate_members(blob, in_off, in_len, frame=_pkg.FRAME_ZLIB):
    """Decode the raw / zlib / gzip members blob[in_off[i]:in_off[i] + in_len[i]] (uint8 tensor; int64 and int32 device
    tensors) whose sizes nobody stated: the size pass, the prefix sum of the sizes, ONE allocation, the framed decode.
    -> (out, out_off, out_len, status): member i is out[out_off[i]:out_off[i] + out_len[i]], status[i] != 0 and
    out_len[i] == 0 where it failed.  A member the size pass refuses (header, stream, gzip ISIZE) takes no room; one that
    fails only in the decode -- a wrong CRC-32 or Adler-32, which the size pass does not examine -- keeps the room of its
    stated size, out_off[i + 1] - out_off[i], holding whatever was decoded.  Nothing visits the host but the total."""
    n = in_off.numel()
    dev = blob.device
    out_size, in_used, status = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    out_off = torch.zeros(n, dtype=torch.int64, device=dev)
    out_len = torch.zeros(n, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev), out_off, out_len, status
    inflate_size_call(blob, in_off, in_len, frame, out_size, in_used, status)
    rc = _pkg.lib().hipdeflate_scan_sizes_dev(_ptr(out_size), n, 0, _ptr(out_off), _ptr(total), _stream())
    _pkg._check(rc, "hipdeflate_scan_sizes_dev")
    out = torch.empty(int(total.item()), dtype=torch.uint8, device=dev)
    inflate_framed_call(blob, in_off, in_len, frame, out, out_off, out_size, out_len, None, None, status)
    return out, out_off, out_len, status


def deflate_dict_call(data, in_off, in_len, level, dictionary, out, out_stride, out_cap, out_len, crc, status):
    """one hipdeflate_batch_deflate_dict_dev over device tensors (dictionary: a uint8 tensor, or None)"""
    dict_len = 0 if dictionary is None else dictionary.numel()
    rc = _pkg.lib().hipdeflate_batch_deflate_dict_dev(_ptr(data), _ptr(in_off), _ptr(in_len), in_off.numel(), level,
                                                      _ptr(dictionary) if dict_len else None, dict_len, _ptr(out), out_stride,
                                                      out_cap, _ptr(out_len), _ptr(crc), _ptr(status), _stream())
    _pkg._check(rc, "hipdeflate_batch_deflate_dict_dev")


def inflate_dict_call(blob, in_off, in_len, frame, dictionary, out, out_off, out_cap, out_len, check, in_used, status):
    """one hipdeflate_batch_inflate_dict_dev over device tensors (dictionary, check, in_used: a tensor or None)"""
    dict_len = 0 if dictionary is None else dictionary.numel()
    rc = _pkg.lib().hipdeflate_batch_inflate_dict_dev(_ptr(blob), _ptr(in_off), _ptr(in_len), in_off.numel(), frame,
                                                      _ptr(dictionary) if dict_len else None, dict_len, _ptr(out), _ptr(out_off),
                                                      _ptr(out_cap), _ptr(out_len), _ptr(check), _ptr(in_used), _ptr(status),
                                                      _stream())
    _pkg._check(rc, "hipdeflate_batch_inflate_dict_dev")


def deflate_dict(data, in_off, in_len, dictionary, level=6):
    """Compress the blocks data[in_off[i]:in_off[i] + in_len[i]] (uint8 tensor; int64 and int32 device tensors) against one
    preset dictionary (uint8 tensor): raw members, each for zlib.decompressobj(-15, zdict=dictionary).
    -> (slots, slot, out_len, crc, status): member i is slots[i * slot:i * slot + out_len[i]]."""
    n = in_off.numel()
    dev = data.device
    slot = int(_pkg.lib().hipdeflate_bound(int(in_len.max().item()) if n else 0, level))
    slots = torch.empty(max(n * slot, 16), dtype=torch.uint8, device=dev)
    out_len, crc, status = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    deflate_dict_call(data, in_off, in_len, level, dictionary, slots, slot, slot, out_len, crc, status)
    return slots, slot, out_len, crc, status


def inflate_dict(blob, in_off, in_len, dictionary, frame=_pkg.FRAME_RAW, out_cap=None):
    """Decode the raw or zlib members blob[in_off[i]:in_off[i] + in_len[i]] that were written with the preset dictionary.
    out_cap: an int32 tensor of rooms; None: 64 KiB each.  -> (out, out_off, out_len, status)"""
    n = in_off.numel()
    dev = blob.device
    if out_cap is None:
        out_cap = torch.full((n,), 65536, dtype=torch.int32, device=dev)
    rooms = (out_cap.to(torch.int64) + 15) & ~15
    out_off = torch.cumsum(rooms, 0) - rooms
    out = torch.empty(max(int(rooms.sum().item()), 16), dtype=torch.uint8, device=dev)
    out_len, status = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(2))
    if n:
        inflate_dict_call(blob, in_off, in_len, frame, dictionary, out, out_off, out_cap, out_len, None, None, status)
    return out, out_off, out_len, status


def block_table(total_bytes, block_size, device="cuda"):
    nb = (total_bytes + block_size - 1) // block_size
    off = torch.arange(nb, dtype=torch.int64, device=device) * block_size
    ln = torch.clamp(total_bytes - off, max=block_size).to(torch.int32)
    return off, ln


def to_numpy_u32(t):
    return t.cpu().numpy().view(np.uint32)
