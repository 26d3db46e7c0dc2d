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

    def index(self, blob):
        """blob: uint8 tensor, 16-byte aligned -> MemberSummary; the tables hold min(nmembers, max_members) entries"""
        summary = _pkg.MemberSummary()
        rc = _pkg.lib().hipdeflate_index_members_dev(
            _ptr(blob), blob.numel(), self.max_members, _ptr(self.in_off), _ptr(self.in_len), _ptr(self.out_size),
            _ptr(self.out_off), _ptr(self.crc_want), ctypes.byref(summary), _stream())
        _pkg._check(rc, "hipdeflate_index_members_dev")
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
            why = {1: "not a member", 2: "member cut off", 3: "more members than max_members = %d" % self.max_members}
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


def inflate_container(blob):
    """uint8 tensor holding a whole container file -> uint8 tensor of its contents; nothing visits the host.
    Two passes over the blob: a table of no entries answers status 3 and the number of members the stream has, the
    table of that size then gives out_bytes and is the one the inflate runs on."""
    d = DeviceInflate(DeviceInflate(0, blob.device).index(blob).nmembers, blob.device)
    s = d.index(blob)
    out = torch.empty(s.out_bytes, dtype=torch.uint8, device=blob.device)
    d.run(blob, out, s)
    return out


def device_inflate(comp, in_off, in_len, out, out_off, out_cap, out_len, crc, status):
    nb = in_off.numel()
    rc = _pkg.lib().hipdeflate_batch_inflate_dev(_ptr(comp), _ptr(in_off), _ptr(in_len), nb, _ptr(out), _ptr(out_off),
                                                 _ptr(out_cap), _ptr(out_len), _ptr(crc), _ptr(status), _stream())
    _pkg._check(rc, "hipdeflate_batch_inflate_dev")


def block_table(total_bytes, block_size, device="cuda"):
    nb = (total_bytes + block_size - 1) // block_size
    off = torch.arange(nb, dtype=torch.int64, device=device) * block_size
    ln = torch.clamp(total_bytes - off, max=block_size).to(torch.int32)
    return off, ln


def to_numpy_u32(t):
    return t.cpu().numpy().view(np.uint32)
