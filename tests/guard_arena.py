"""
Device buffers carved between guard bands, for the third sweep over tests/caller_stream_cases.py (memory extent and
alignment; tests/test_gpu_guard_bands.py).  TEST INFRASTRUCTURE ONLY; nothing here touches the GPU at import, and torch is
imported inside functions only.  tests/test_guard_arena.py checks this file on the CPU.

Every other suite takes its buffers from torch.empty: blocks aligned to 512 bytes, sizes rounded up, small blocks packed into
shared segments.  A read or a store a few elements outside such a buffer lands in mapped memory and nobody looks there, and a
kernel that works only at that alignment is never shown another.  carve() gives a case the same tensors as Case.alloc, each a
contiguous view into a torch.uint8 allocation of its own:

    [ front guard | pad to the start | payload | back guard ]

    start "sixteen"   the payload begins 16 bytes after a 256-byte boundary: 16-byte aligned and no better
    start "element"   the payload begins one element after a 256-byte boundary: aligned to its element type and no better
                      (8 bytes off for the 64-bit types, 4 for the 32-bit ones, 2 for the 16-bit ones, 1 for bytes)
    fill              the byte in every guard and pad byte, 0xFF or 0x00: with 0xFF every fp64 guard element is a NaN and
                      every integer guard its largest (or -1), with 0x00 they are zeros -- a result that a value from outside
                      a buffer has entered differs between the two

`start` is one of the two names, or a dict name -> start whose key "*" gives the start of every tensor it does not name.
feed, fill_outputs, snapshot and differing of caller_stream_cases.py work on the carved tensors unchanged.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import caller_stream_cases as R  # noqa: E402

# A condition, not a measurement: 4 KiB is one row of 512 doubles, longer than any row, tile or vector of the registry's
# shapes (Nreg 17 / 33, U 3 / 7, T <= 136), so an access one row, tile or vector outside a buffer lands in a guard.
GUARD = 4096
BOUNDARY = 256
STARTS = ("sixteen", "element")
FILLS = (0xFF, 0x00)


def start_offset(start, itemsize):
    """bytes between the 256-byte boundary and the payload"""
    assert start in STARTS, start
    return 16 if start == "sixteen" else int(itemsize)


class Band(object):
    """one tensor of an arena: its allocation, the payload's extent in it and the view"""

    def __init__(self, name, raw, lo, nbytes, view):
        (self.name, self.raw, self.lo, self.nbytes, self.view) = (name, raw, int(lo), int(nbytes), view)
        self.hi = self.lo + self.nbytes                    # the back guard is raw[hi : hi + GUARD], the end of raw

    def extent(self):
        """(address of the allocation, of the payload, of the payload's end, of the allocation's end)"""
        base = self.raw.data_ptr()
        return (base, base + self.lo, base + self.hi, base + self.raw.numel())


class Arena(object):
    def __init__(self, device, fill):
        assert fill in FILLS, fill
        (self.device, self.fill, self.bands) = (device, int(fill), {})

    def add(self, name, shape, dtype, start):
        """a contiguous tensor of this shape and (torch) dtype at the start asked for, guards and pad filled"""
        import torch
        assert name not in self.bands, name
        itemsize = torch.empty(0, dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        off = start_offset(start, itemsize)
        raw = torch.empty(GUARD + 2 * BOUNDARY + nbytes + GUARD, dtype=torch.uint8, device=self.device)
        base = raw.data_ptr()
        lo = GUARD + (off - (base + GUARD)) % BOUNDARY     # the first address >= base + GUARD that is `off` past a boundary
        raw = raw[:lo + nbytes + GUARD]
        raw[:lo].fill_(self.fill)
        raw[lo + nbytes:].fill_(self.fill)
        assert lo % itemsize == 0, "the allocator's block is not aligned to the element type"
        view = raw[lo:lo + nbytes].view(dtype).view(tuple(int(n) for n in shape))
        assert view.is_contiguous() and view.data_ptr() == base + lo and view.data_ptr() % BOUNDARY == off
        self.bands[name] = Band(name, raw, lo, nbytes, view)
        return view

    def names_start_at(self, k):
        """the names whose payload begins k bytes after a 256-byte boundary"""
        return sorted(n for (n, b) in self.bands.items() if b.view.data_ptr() % BOUNDARY == k)

    def check(self):
        """
        The guard and pad bytes that changed: a list of (name, side, offset), one entry per tensor and side, with the FIRST
        changed byte of that side.  side "front": offset < 0, counted from the payload's first byte (-1 is the byte directly
        before it); side "back": offset >= 0, counted from the first byte after the payload.
        """
        found = []
        for name in sorted(self.bands):
            b = self.bands[name]
            for (side, region) in (("front", b.raw[:b.lo]), ("back", b.raw[b.hi:])):
                changed = (region != self.fill).nonzero()
                if changed.numel():
                    first = int(changed[0, 0])
                    found.append((name, side, first - b.lo if side == "front" else first))
        return found


HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "fcdiff_hip.h")


def alignment_contract(text=None):
    """
    The alignment table of include/fcdiff_hip.h: ({entry point: [arguments that must be 16-byte aligned]},
    {entry point: [arguments whose address chooses the path]}), from its "align16:" and "by-address:" lines.
    """
    import re
    if text is None:
        with open(HEADER) as fh:
            text = fh.read()
    tables = {"align16": {}, "by-address": {}}
    for m in re.finditer(r"^\s*\*\s+(align16|by-address):\s+(fcd_\w+)\(([^)]*)\)", text, flags=re.M):
        assert m.group(2) not in tables[m.group(1)], m.group(2)
        tables[m.group(1)][m.group(2)] = [a.strip() for a in m.group(3).split(",")]
    return tables["align16"], tables["by-address"]


def carve(case, size, device, start, fill):
    """(din, dout, arena) with the contract of Case.alloc: the tensors of the case at this size, uninitialised"""
    spec = case.spec(size)
    arena = Arena(device, fill)

    def start_of(name):
        return start if isinstance(start, str) else start.get(name, start["*"])
    din = dict((k, arena.add(k, v.shape, R._tdtype(v.dtype), start_of(k))) for (k, v) in spec["inputs"].items())
    (din["_host"], din["_inout"]) = (spec["host"], tuple(spec["inout"]))
    dout = dict((k, arena.add(k, shape, R._tdtype(dtype), start_of(k))) for (k, (shape, dtype)) in spec["outputs"].items())
    return din, dout, arena
