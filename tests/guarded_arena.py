"""Guarded arenas for the batched API's engines (test infrastructure).

One call's device buffers are laid out in ONE allocation: every buffer sits
between two guard regions of at least GUARD canary bytes and starts at exactly
the minimum alignment include/razor_fec.h documents for it ("Alignment": the
address is a multiple of `align` and of nothing larger), as a caller who
sub-allocates one arena would pass them.  After the call the arena checks

  * every guard byte (a store one chunk past any buffer lands in one),
  * every input-only buffer, byte for byte against its snapshot,
  * for an in-place recover, every received segment's slot and header.

The layout and the checks only slice, compare and reduce arrays, so they run on
numpy arrays (OracleArenaEngine below: the CPU run, and the self-test that the
checks can fail) and on torch tensors in HBM (GpuEngine, gpu_engine.py) alike:
the comparison happens where the memory is and nothing is downloaded unless a
check fails.

ArenaEngine implements the engine interface of parity_cases.py (encode,
recover, recover_out) over such arenas; a subclass supplies the memory
(backend) and the raw calls on addresses.
"""
from __future__ import annotations

import numpy as np

GUARD = 4096
# differs from every pre-fill the engines and cases use: 0x5A (encode outputs), 0x3C (dense outputs), 0xEE
# (recovered masks), 0x77 (packed records), 0xA5 (erased slots), 0x00 and 0xFF
CANARY = 0xC7
PREFILLS = (0x5A, 0x3C, 0xEE, 0x77, 0xA5)
assert CANARY not in PREFILLS + (0x00, 0xFF)

HDR_BYTES = 20

# minimum alignment of each pointer of the batched API (razor_fec.h, "Alignment")
ALIGN = {"shards": 16, "parity": 16, "out_shards": 16, "workspace": 16, "packed": 16,
         "hdr": 4, "meta": 4, "out_hdr": 4, "present": 8, "parity_present": 8, "recovered": 8,
         "fec_size": 2, "status": 1, "out_index": 1}


class Buf:
    """One buffer of a call.  init: bytes to upload (any numpy array), or a fill
    byte.  role: "in" (the call must leave it byte-identical), "out", "inout"
    or "scratch"."""

    def __init__(self, name, nbytes, init, role, align=None):
        assert role in ("in", "out", "inout", "scratch")
        self.name, self.nbytes, self.init, self.role = name, int(nbytes), init, role
        self.align = ALIGN[name] if align is None else align
        self.off = None


class NumpyBackend:
    """Host memory (the oracle's run)."""

    def full(self, n, byte):
        return np.full(n, byte, np.uint8)

    def address(self, mem):
        return mem.ctypes.data

    def put(self, view, a):
        view[...] = a

    def fill(self, view, byte):
        view[...] = byte

    def asarray(self, a):
        return np.ascontiguousarray(a)

    def clone(self, view):
        return view.copy()

    def numpy(self, view):
        return np.array(view)

    def sync(self):
        pass


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Arena:
    def __init__(self, backend, bufs):
        self.be = backend
        self.bufs = {b.name: b for b in bufs}
        assert len(self.bufs) == len(bufs)
        total = GUARD + sum(b.nbytes + GUARD + 3 * b.align for b in bufs)
        self.mem = backend.full(total, CANARY)
        base = backend.address(self.mem)
        off = 0
        self.guards = []  # (buffer, side, start, end)
        prev = None
        for b in bufs:
            lo = off
            a = base + off + GUARD
            a += (-a) % (2 * b.align) + b.align  # a multiple of align, an odd one: aligned to nothing larger
            b.off = a - base
            assert (base + b.off) % b.align == 0 and (base + b.off) % (2 * b.align) != 0
            assert b.off - lo >= GUARD
            # the region between two buffers guards both: named after the one it precedes and, from its start,
            # after the one it follows
            self.guards.append((b.name, "before", lo, b.off, prev))
            off = b.off + b.nbytes
            prev = b.name
        assert total - off >= GUARD
        self.guards.append((prev, "after", off, total, None))
        self.base = base
        self.snap = {}
        for b in bufs:
            v = self.view(b.name)
            if isinstance(b.init, (int, np.integer)):
                if b.nbytes:
                    backend.fill(v, int(b.init))
            else:
                raw = _bytes(b.init)
                assert raw.size == b.nbytes, (b.name, raw.size, b.nbytes)
                if b.nbytes:
                    backend.put(v, raw)
            if b.role in ("in", "inout"):
                self.snap[b.name] = backend.clone(v)
        self.rows = []  # (buffer, row bytes, kept-rows mask in backend memory, what)

    def view(self, name):
        b = self.bufs[name]
        return self.mem[b.off:b.off + b.nbytes]

    def ptr(self, name):
        return self.base + self.bufs[name].off

    def get(self, name, dtype, shape):
        return self.be.numpy(self.view(name)).view(dtype).reshape(shape)

    def keep_rows(self, name, row_bytes, keep, what):
        """Rows of an in/out buffer (row_bytes each) that the call must leave alone: keep[r] true."""
        assert self.bufs[name].role == "inout" and self.bufs[name].nbytes == len(keep) * row_bytes
        self.rows.append((name, row_bytes, self.be.asarray(np.ascontiguousarray(keep, bool)), what))

    # -- the checks -----------------------------------------------------------
    def _flags(self):
        flags = []
        for name, side, a, b, _ in self.guards:
            flags.append(("guard", name, side, (self.mem[a:b] != CANARY).any()))
        for name, b in self.bufs.items():
            if b.role == "in" and b.nbytes:
                flags.append(("input", name, None, (self.view(name) != self.snap[name]).any()))
        for name, rb, keep, what in self.rows:
            changed = (self.view(name) != self.snap[name]).reshape(-1, rb).any(1)
            flags.append(("rows", name, what, (changed & keep).any()))
        return flags

    def check(self, where):
        """Raises AssertionError naming every damaged buffer.  One reduction per region where the memory is, one
        synchronising read of the combined flag; downloads happen only to describe a failure."""
        flags = self._flags()
        bad = flags[0][3]
        for f in flags[1:]:
            bad = bad | f[3]
        if not bool(bad):
            return
        msgs = []
        for kind, name, side, f in flags:
            if not bool(f):
                continue
            if kind == "guard":
                _, _, a, b, prev = next(g for g in self.guards if g[0] == name and g[1] == side)
                d = np.nonzero(self.be.numpy(self.mem[a:b]) != CANARY)[0]
                # a region between two buffers guards both: damage in its first half is past the end of the
                # buffer it follows, damage in its second half before the start of the one it precedes
                mid = (b - a) // 2 if prev is not None and side == "before" else (b - a if side == "after" else 0)
                lo, hi = d[d < mid], d[d >= mid]
                if len(lo):
                    msgs.append(f"guard after {prev if side == 'before' else name}: {len(lo)} bytes damaged, the "
                                f"first at offset {int(lo[0])} past its end")
                if len(hi):
                    msgs.append(f"guard before {name}: {len(hi)} bytes damaged, the first at offset "
                                f"{int(hi[0]) - (b - a)} from its start")
            elif kind == "input":
                d = np.nonzero(self.be.numpy(self.view(name)) != self.be.numpy(self.snap[name]))[0]
                msgs.append(f"input {name} was written: {len(d)} bytes differ, the first at offset {int(d[0])}")
            else:
                rb = next(r[1] for r in self.rows if r[0] == name)
                keep = self.be.numpy(next(r[2] for r in self.rows if r[0] == name))
                d = (self.be.numpy(self.view(name)) != self.be.numpy(self.snap[name])).reshape(-1, rb)
                rows = np.nonzero(d.any(1) & keep)[0]
                r0 = int(rows[0])
                msgs.append(f"{side} of {name} was written: {len(rows)} rows differ, the first row {r0} at byte "
                            f"{int(np.nonzero(d[r0])[0][0])}")
        raise AssertionError(f"{where}: " + "; ".join(msgs))


def present_rows(present, k):
    """[G*k] bool: segment i of group g was received (present [G][2] u64)."""
    p = np.ascontiguousarray(present, np.uint64).reshape(-1, 2)
    bits = np.arange(k, dtype=np.uint64)
    lo = (p[:, :1] >> np.minimum(bits, np.uint64(63))[None, :]) & np.uint64(1)
    hi = (p[:, 1:] >> (np.maximum(bits, np.uint64(64)) - np.uint64(64))[None, :]) & np.uint64(1)
    return np.where(bits[None, :] < 64, lo, hi).astype(bool).reshape(-1)


class ArenaEngine:
    """encode / recover / recover_out (parity_cases.py's engine interface, numpy
    in, numpy out) with every buffer of the call in a guarded arena.  Subclasses
    set self.be and implement _encode / _recover / _recover_out / _workspace_size
    over an Arena's addresses.  `mutate` (tests): called with (arena, call name)
    after the call and before the checks.  last_path: the dispatch tag of the
    call (0 where the engine has none)."""

    be = None
    mutate = None
    last_path = 0
    random_workspace = False
    HDR = None  # numpy dtype of rfec_hdr

    def _finish(self, A, what):
        self.be.sync()
        if self.mutate is not None:
            self.mutate(A, what)
        A.check(what)

    def _workspace(self, plan, G):
        n = max(16, self._workspace_size(plan, G))
        if self.random_workspace:
            return np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        return 0

    def encode(self, plan, shards, hdr, capacity):
        G, k, stride = shards.shape
        n = plan.n_lines
        A = Arena(self.be, [Buf("shards", shards.size, shards, "in"), Buf("hdr", G * k * HDR_BYTES, hdr, "in"),
                            Buf("parity", G * n * stride, 0x5A, "out"), Buf("meta", G * n * HDR_BYTES, 0x5A, "out"),
                            Buf("fec_size", G * n * 2, 0, "out"), Buf("status", G * n, 7, "out")])
        self._encode(plan, G, stride, capacity, A)
        self._finish(A, "encode")
        return (A.get("parity", np.uint8, (G, n, stride)), A.get("meta", self.HDR, (G, n)),
                A.get("fec_size", np.uint16, (G, n)), A.get("status", np.int8, (G, n)))

    def _recover_bufs(self, plan, shards, hdr, present, parity, meta, fsize, pp, role):
        G, k, stride = shards.shape
        n = plan.n_lines
        ws = self._workspace(plan, G)
        nws = max(16, self._workspace_size(plan, G))
        return [Buf("shards", shards.size, shards, role), Buf("hdr", G * k * HDR_BYTES, hdr, role),
                Buf("present", G * 16, np.ascontiguousarray(present, np.uint64), "in"),
                Buf("parity", G * n * stride, parity, "in"), Buf("meta", G * n * HDR_BYTES, meta, "in"),
                Buf("fec_size", G * n * 2, np.ascontiguousarray(fsize, np.uint16), "in"),
                Buf("parity_present", G * 8, np.ascontiguousarray(pp, np.uint64), "in"),
                Buf("recovered", G * 16, 0xEE, "out"), Buf("workspace", nws, ws, "scratch")]

    def recover(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity):
        G, k, stride = shards.shape
        A = Arena(self.be, self._recover_bufs(plan, shards, hdr, present, parity, meta, fsize, pp, "inout"))
        keep = present_rows(present, k)
        A.keep_rows("shards", stride, keep, "a received segment")
        A.keep_rows("hdr", HDR_BYTES, keep, "a received segment's header")
        self._recover(plan, G, stride, capacity, A)
        self._finish(A, "recover")
        return (A.get("shards", np.uint8, (G, k, stride)), A.get("hdr", self.HDR, (G, k)),
                A.get("recovered", np.uint64, (G, 2)))

    def recover_out(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity, per_group):
        """rfec_recover_batch_out: returns (out_shards [G][E][stride], out_hdr
        [G][E], out_index [G][E], recovered [G][2]); the shards and headers are
        inputs here."""
        G, k, stride = shards.shape
        E = per_group
        A = Arena(self.be, self._recover_bufs(plan, shards, hdr, present, parity, meta, fsize, pp, "in") +
                  [Buf("out_shards", G * E * stride, 0x3C, "out"), Buf("out_hdr", G * E * HDR_BYTES, 0x3C, "out"),
                   Buf("out_index", G * E, 0x3C, "out")])
        self._recover_out(plan, G, stride, capacity, E, A)
        self._finish(A, "recover_out")
        return (A.get("out_shards", np.uint8, (G, E, stride)), A.get("out_hdr", self.HDR, (G, E)),
                A.get("out_index", np.uint8, (G, E)), A.get("recovered", np.uint64, (G, 2)))


class OracleArenaEngine(ArenaEngine):
    """The CPU oracle (oracle/rfec_oracle.c) behind the same arenas, restating the
    slot contract of razor_fec.h ("Slot tails"): the oracle computes whole slots
    of `stride` bytes; the API works on the ceil(capacity / 16) chunks of a slot,
    so the bytes of a written slot from there to the stride keep what they held."""

    def __init__(self, oracle):
        import pyoracle as po
        self.o, self.po = oracle, po
        self.be = NumpyBackend()
        self.HDR = po.HDR_DTYPE

    def _workspace_size(self, plan, G):
        return 16

    def _plan(self, plan):
        import ctypes as C
        return C.byref(self.po._as_oracle_plan(plan))

    @staticmethod
    def _cd16(capacity):
        return 16 * ((capacity + 15) // 16) if capacity else 16

    def _encode(self, plan, G, stride, capacity, A):
        before = A.get("parity", np.uint8, (G, plan.n_lines, stride))
        self.o.lib.oracle_encode_batch(self._plan(plan), G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "parity", "meta", "fec_size", "status")))
        w = self._cd16(capacity)
        if w < stride and A.bufs["parity"].nbytes:
            A.view("parity").reshape(G, plan.n_lines, stride)[:, :, w:] = before[:, :, w:]

    def _recover(self, plan, G, stride, capacity, A):
        k = plan.k
        before = A.get("shards", np.uint8, (G, k, stride))
        self.o.lib.oracle_recover_batch(self._plan(plan), G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "recovered")))
        w = self._cd16(capacity)
        if w < stride:
            A.view("shards").reshape(G, k, stride)[:, :, w:] = before[:, :, w:]

    def _recover_out(self, plan, G, stride, capacity, E, A):
        before = A.get("out_shards", np.uint8, (G, E, stride))
        self.o.lib.oracle_recover_batch_out(self._plan(plan), G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "recovered")), E,
            *(A.ptr(n) for n in ("out_shards", "out_hdr", "out_index")))
        w = self._cd16(capacity)
        if w < stride:
            A.view("out_shards").reshape(G, E, stride)[:, :, w:] = before[:, :, w:]
