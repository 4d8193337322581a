"""Guard bands round the outputs of a call: does it write outside the memory it was given?

One allocation -- device memory for `Arena`, a ctypes buffer for `HostArena` -- is carved into named regions.  A region
starts on a 16-byte boundary (the library refuses device pointers that are not 16-byte aligned) and its rear guard starts
at start + nbytes, not at the next aligned address: the byte after a 3-byte `is_one` output is a guard byte.  Every byte of
the arena that lies in no region is a guard byte, and between two regions, before the first and after the last there are at
least GUARD of them.

How GUARD was chosen.  A guard must be at least 4 KiB and at least as wide as the largest span one workgroup of the kernel
under test writes, so that a workgroup that runs one whole tile too far still lands inside it.  The widest such spans are
  * the transform, 2^kNttTileLog = 1024 records of 32 B per workgroup (ntt.hip.h)                          32 KiB
  * the radix sort, kRadixTile = 256 * kRadixItems = 4096 pairs of 8 B per workgroup (launch.h)            32 KiB
  * the point kernels, 64 lanes of one record each, the largest record being a GT one of 384 B             24 KiB
  * the Fr scans, 2^kFrTileLog = 512 records of 32 B per tile (fr_vec.hip.h)                               16 KiB
  * the Fr maps, kFrMapThreads = 256 records of 32 B (fr_vec.hip.h)                                         8 KiB
and one width for all keeps the harness simple: GUARD = 32 KiB.

The fill.  commit() writes the whole arena, guards and outputs alike, from a seeded random.Random byte stream (never a
constant byte: a kernel that writes zeros or 0xFF past its end is seen as well as any other), lays the inputs over it and
uploads it; call it before every call under test.

verify() reads the whole arena back once and raises GuardError if a guard byte, a byte of a read-only region, or a byte of
an output region outside the `writable` ranges it was registered with differs from what commit() wrote.  The message names
the region, the side, the first and last changed offset relative to the region's start (front) or end (rear) and the
number of changed bytes: `rear +0..+31, 32 bytes` is one extra record, `rear +0..+12, 13 bytes` a length rounded up to 16.
unchanged() asserts that the whole arena, outputs included, is as commit() left it (a refused call).

What this cannot see: reads past the end of an input, writes that land further away than GUARD, and writes into memory
the library owns (the workspaces of a ctx)."""
import ctypes
import random

GUARD = 32 * 1024
ALIGN = 16


class GuardError(AssertionError):
    pass


class Region:
    def __init__(self, name, off, nbytes, data, readonly, writable):
        self.name, self.off, self.nbytes, self.data, self.readonly, self.writable = name, off, nbytes, data, readonly, writable
        self.ptr = None

    @property
    def end(self):
        return self.off + self.nbytes


def _changed(a, b, lo, hi):
    """offsets in [lo, hi) at which a and b differ"""
    if a[lo:hi] == b[lo:hi]:
        return []
    return [i for i in range(lo, hi) if a[i] != b[i]]


class _ArenaBase:
    def __init__(self, guard=GUARD):
        assert guard >= 4096
        self.guard, self.regions, self.size, self.base, self.image, self.back, self.seed = guard, {}, guard, None, None, None, 0

    # ---- layout --------------------------------------------------------------------------------------------------------------
    def add(self, name, nbytes=None, data=None, readonly=False, writable=None):
        """A region of nbytes (or of len(data)) bytes; data is laid over the fill at commit().  readonly: verify() holds every
        byte to what commit() wrote.  writable: (offset, length) ranges of an output region the call may write; the rest of
        the region (the gaps of a strided output) is held like a guard.  Returns the region; .ptr is set by commit()."""
        assert self.base is None and name not in self.regions, name
        nbytes = len(data) if nbytes is None else nbytes
        assert data is None or len(data) <= nbytes
        r = Region(name, self.size, nbytes, data, readonly, writable)
        self.regions[name] = r
        self.size = -(-(r.end + self.guard) // ALIGN) * ALIGN          # the next region's start; the last one's rear guard
        return r

    def commit(self, seed=None):
        """allocate (the first time), fill everything from the seeded stream, lay the inputs over it, upload"""
        if self.base is None:
            self.total = max(32, self.size)
            self.base = self._alloc(self.total)
            for r in self.regions.values():
                r.ptr = self.base + r.off
        self.seed = self.seed + 1 if seed is None else seed
        image = bytearray(random.Random(0x6A5D0000 + self.seed).randbytes(self.total))
        for r in self.regions.values():
            if r.data is not None:
                image[r.off:r.off + len(r.data)] = r.data
        self.image, self.back = bytes(image), None
        self._upload(self.image)
        return self

    def set(self, name, data):
        """new contents for a region from the next commit() on"""
        assert len(data) <= self.regions[name].nbytes
        self.regions[name].data = data

    def ptr(self, name):
        return self.regions[name].ptr

    # ---- checks --------------------------------------------------------------------------------------------------------------
    def _protected(self):
        """(lo, hi, region, side) of every span verify() holds to the fill; side offsets are relative to `origin`"""
        spans, rs = [], sorted(self.regions.values(), key=lambda r: r.off)
        for k, r in enumerate(rs):
            lo = rs[k - 1].end if k else 0
            mid = lo if not k else (lo + r.off + 1) // 2                 # a gap is shared: each byte goes to the nearer region
            spans.append((mid, r.off, r, "front", r.off))
            if r.readonly:
                spans.append((r.off, r.end, r, "read-only", r.off))
            elif r.writable is not None:
                at = 0
                for off, length in sorted(r.writable):
                    spans.append((r.off + at, r.off + off, r, "gap", r.off))
                    at = off + length
                spans.append((r.off + at, r.end, r, "gap", r.off))
            hi = rs[k + 1].off if k + 1 < len(rs) else self.total
            mid = hi if k + 1 == len(rs) else (r.end + hi + 1) // 2
            spans.append((r.end, mid, r, "rear", r.end))
        return spans

    def verify(self):
        """read the arena back; raise GuardError for every protected span with a changed byte; return self"""
        self.back = self._download()
        assert len(self.back) == self.total
        found = []
        for lo, hi, r, side, origin in self._protected():
            bad = _changed(self.back, self.image, lo, hi)
            if bad:
                found.append("region '%s' (%d bytes) %s: offsets %+d..%+d changed, %d bytes"
                             % (r.name, r.nbytes, side, bad[0] - origin, bad[-1] - origin, len(bad)))
        if found:
            raise GuardError("; ".join(found))
        return self

    def unchanged(self):
        """the whole arena, outputs included, is as commit() left it"""
        self.back = self._download()
        if self.back != self.image:
            bad = _changed(self.back, self.image, 0, self.total)
            hit = [r.name for r in self.regions.values() if any(r.off <= i < r.end for i in (bad[0], bad[-1]))]
            raise GuardError("a refused call wrote: arena offsets %d..%d changed, %d bytes (regions %s)"
                             % (bad[0], bad[-1], len(bad), hit or "none: guard bytes"))
        return self

    def get(self, name, nbytes=None, off=0):
        """bytes of a region as verify() / unchanged() read them back"""
        r = self.regions[name]
        nbytes = r.nbytes - off if nbytes is None else nbytes
        return self.back[r.off + off:r.off + off + nbytes]

    def filled(self, name, nbytes=None, off=0):
        """the same bytes as commit() wrote them"""
        r = self.regions[name]
        nbytes = r.nbytes - off if nbytes is None else nbytes
        return self.image[r.off + off:r.off + off + nbytes]


class Arena(_ArenaBase):
    """guard bands in device memory of one MsmConfig"""

    def __init__(self, cfg, guard=GUARD):
        super().__init__(guard)
        self.cfg = cfg

    def _alloc(self, nbytes):
        base = self.cfg.alloc(nbytes)
        assert base % ALIGN == 0
        return base

    def _upload(self, image):
        self.cfg.to_device(self.base, image)

    def _download(self):
        return self.cfg.to_host(self.base, self.total)

    def poke(self, offset, data):
        """write bytes at an arena offset behind the harness's back (its own self-check)"""
        self.cfg.to_device(self.base + offset, data)

    def close(self):
        if self.base is not None:
            self.cfg.free(self.base)
            self.base = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HostArena(_ArenaBase):
    """the same over one ctypes buffer; a region's .ptr is an address to hand to a C function as c_void_p"""

    def _alloc(self, nbytes):
        self.buf = ctypes.create_string_buffer(nbytes + ALIGN)
        return -(-ctypes.addressof(self.buf) // ALIGN) * ALIGN

    def _upload(self, image):
        ctypes.memmove(self.base, image, len(image))

    def _download(self):
        return ctypes.string_at(self.base, self.total)

    def poke(self, offset, data):
        ctypes.memmove(self.base + offset, data, len(data))

    def close(self):
        self.base = self.buf = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Out:
    """placeholder for an output argument of guarded(): nbytes, or data for an in-place argument; writable as in add();
    host: the argument is host memory of a call whose other buffers are device memory"""

    def __init__(self, nbytes=None, data=None, writable=None, host=False):
        self.nbytes, self.data, self.writable, self.host = nbytes, data, writable, host


class In:
    """placeholder for a read-only input argument of guarded()"""

    def __init__(self, data, host=False):
        self.data, self.host = data, host


class At:
    """a placeholder's region `shift` bytes in: a misaligned or partly overlapping pointer of a call that must be refused"""

    def __init__(self, placeholder, shift):
        self.placeholder, self.shift = placeholder, shift


def guarded(arena, fn, *args, ok=0, seed=None, host_arena=None):
    """Call the C function fn with every Out / In argument replaced by the address of a region of `arena` (a fresh arena:
    regions are named by the function and the argument's position, 0-based; placeholders with host=True go to `host_arena`), after commit(); assert it
    returns `ok`, verify() the guards and return the bytes of every Out in argument order.  The same placeholder object may
    stand at two positions (an in-place call)."""
    seen, call, shifts = {}, [], {}
    label = getattr(fn, "__name__", "call")
    for k, a in enumerate(args):
        if isinstance(a, At):
            shifts[k], a = a.shift, a.placeholder
        if isinstance(a, (Out, In)):
            if id(a) not in seen:
                where = host_arena if a.host else arena
                if isinstance(a, In):
                    seen[id(a)] = (where, where.add("%s arg %d" % (label, k), data=a.data, readonly=True))
                else:
                    seen[id(a)] = (where, where.add("%s arg %d" % (label, k), a.nbytes, a.data, writable=a.writable))
            call.append(seen[id(a)][1])
        else:
            call.append(a)
    used = [x for x in (arena, host_arena) if x is not None and x.regions]
    for x in used:
        x.commit(seed)
    st = fn(*[ctypes.c_void_p(a.ptr + shifts.get(k, 0)) if isinstance(a, Region) else a for k, a in enumerate(call)])
    assert st == ok, "status %d, expected %d" % (st, ok)
    for x in used:
        x.verify() if ok == 0 else x.unchanged()
    outs, done = [], set()
    for a in args:
        a = a.placeholder if isinstance(a, At) else a
        if isinstance(a, Out) and id(a) not in done:
            done.add(id(a))
            where, region = seen[id(a)]
            outs.append(where.get(region.name))
    return outs
