"""Runs the product (librazor_fec.so, HIP kernels) on numpy inputs: uploads to
HBM with torch (allocator only), calls the C ABI, downloads the results.  The
batched API's engine (GpuEngine) keeps each call's buffers in one guarded arena
(guarded_arena.py) and checks guards, inputs and received segments after it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

import guarded_arena as ga
import wire_cases as wc
from razor_amd.fec import HDR_DTYPE, native


def _dev(a: np.ndarray, device) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(device)


def _host(t: torch.Tensor, dtype, shape) -> np.ndarray:
    return t.cpu().numpy().view(dtype).reshape(shape)


class TorchBackend:
    """HBM behind guarded_arena.Arena: one uint8 tensor per arena, compared on the device."""

    def __init__(self, device):
        self.device = device

    def full(self, n, byte):
        return torch.full((n,), byte, dtype=torch.uint8, device=self.device)

    def address(self, mem):
        return mem.data_ptr()

    def put(self, view, a):
        view.copy_(torch.from_numpy(a))

    def fill(self, view, byte):
        view.fill_(byte)

    def asarray(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def clone(self, view):
        return view.clone()

    def numpy(self, view):
        return view.cpu().numpy()

    def sync(self):
        torch.cuda.synchronize(self.device)


class GpuEngine(ga.ArenaEngine):
    """The batched API on numpy inputs.  Every call lays its device buffers out
    in one guarded arena (guarded_arena.py): each between canary guards, each at
    exactly the alignment razor_fec.h documents; after the call the guards, the
    input-only buffers and (in place) the received segments are checked on the
    device.  last_path: the dispatch tag of the call's last launch
    (rfec_internal.h RFEC_PATH)."""

    HDR = HDR_DTYPE

    def __init__(self, video_size=1000, device="cuda:0", tuning=0, random_workspace=False):
        self.lib = native(video_size)
        self.lib.lib.rfec_last_path.restype = C.c_uint32
        self.lib.lib.rfec_last_path.argtypes = []
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        self.tuning = tuning
        self.random_workspace = random_workspace  # recover workspace starts as random bytes (not zeroed)

    def _workspace_size(self, plan, G):
        return self.lib.workspace_size(plan, G)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _tuned(self, fn, *args):
        self.lib.set_tuning(self.tuning)
        try:
            fn(*args, self._stream())
            self.last_path = int(self.lib.lib.rfec_last_path())
            torch.cuda.synchronize(self.device)
        finally:
            self.lib.set_tuning(0)

    def _encode(self, plan, G, stride, capacity, A):
        self._tuned(self.lib.encode_batch, plan, G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "parity", "meta", "fec_size", "status")))

    def _recover(self, plan, G, stride, capacity, A):
        self._tuned(self.lib.recover_batch, plan, G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "recovered", "workspace")))

    def _recover_out(self, plan, G, stride, capacity, E, A):
        self._tuned(self.lib.recover_batch_out, plan, G, stride, capacity, *(A.ptr(n) for n in (
            "shards", "hdr", "present", "parity", "meta", "fec_size", "parity_present", "recovered")), E,
            *(A.ptr(n) for n in ("out_shards", "out_hdr", "out_index", "workspace")))

    def recover_packed(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity, per_group, packed=None):
        """rfec_pack_erasures (on the device, unless `packed` gives the records)
        then rfec_recover_packed_out: returns (out_shards, out_hdr, out_index,
        recovered, packed records [G][stride] as built)."""
        G, k, stride = shards.shape
        E = per_group
        n = plan.n_lines
        pks = self.lib.packed_stride(plan, E)
        assert pks > 0
        B = ga.Buf
        bufs = [B("shards", shards.size, shards, "in"), B("parity", G * n * stride, parity, "in")]
        if packed is None:
            bufs += [B("hdr", G * k * ga.HDR_BYTES, hdr, "in"),
                     B("present", G * 16, np.ascontiguousarray(present, np.uint64), "in"),
                     B("meta", G * n * ga.HDR_BYTES, meta, "in"),
                     B("fec_size", G * n * 2, np.ascontiguousarray(fsize, np.uint16), "in"),
                     B("parity_present", G * 8, np.ascontiguousarray(pp, np.uint64), "in"),
                     B("packed", G * pks, 0x77, "out")]
        else:
            assert packed.shape == (G, pks)
            bufs += [B("packed", G * pks, packed, "in")]
        bufs += [B("recovered", G * 16, 0xEE, "out"), B("out_shards", G * E * stride, 0x3C, "out"),
                 B("out_hdr", G * E * ga.HDR_BYTES, 0x3C, "out"), B("out_index", G * E, 0x3C, "out")]
        A = ga.Arena(self.be, bufs)
        st = self._stream()
        if packed is None:
            self.lib.pack_erasures(plan, G, *(A.ptr(n) for n in ("hdr", "present", "meta", "fec_size",
                                                                 "parity_present")), E, A.ptr("packed"), st)
            self.pack_path = int(self.lib.lib.rfec_last_path())
        self.lib.recover_packed_out(plan, G, stride, capacity, A.ptr("shards"), A.ptr("parity"), A.ptr("packed"),
                                    A.ptr("recovered"), E, A.ptr("out_shards"), A.ptr("out_hdr"), A.ptr("out_index"),
                                    st)
        self.last_path = int(self.lib.lib.rfec_last_path())
        self._finish(A, "recover_packed")
        return (A.get("out_shards", np.uint8, (G, E, stride)), A.get("out_hdr", HDR_DTYPE, (G, E)),
                A.get("out_index", np.uint8, (G, E)), A.get("recovered", np.uint64, (G, 2)),
                A.get("packed", np.uint8, (G, pks)))

    def recover_packed_matrix(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity, per_group):
        """rfec_pack_erasures_matrix on the device then rfec_recover_packed_matrix_out, every buffer in one
        guarded arena: returns (out_shards, out_hdr, out_index, recovered, packed records [G][stride])."""
        G, k, stride = shards.shape
        E = per_group
        n = plan.n_lines
        pks = self.lib.packed_matrix_stride(plan, E)
        assert pks > 0 and pks % 64 == 0
        B = ga.Buf
        A = ga.Arena(self.be, [
            B("shards", shards.size, shards, "in"), B("parity", G * n * stride, parity, "in"),
            B("hdr", G * k * ga.HDR_BYTES, hdr, "in"),
            B("present", G * 16, np.ascontiguousarray(present, np.uint64), "in"),
            B("meta", G * n * ga.HDR_BYTES, meta, "in"),
            B("fec_size", G * n * 2, np.ascontiguousarray(fsize, np.uint16), "in"),
            B("parity_present", G * 8, np.ascontiguousarray(pp, np.uint64), "in"),
            B("packed", G * pks, 0x77, "out"), B("recovered", G * 16, 0xEE, "out"),
            B("out_shards", G * E * stride, 0x3C, "out"), B("out_hdr", G * E * ga.HDR_BYTES, 0x3C, "out"),
            B("out_index", G * E, 0x3C, "out")])
        st = self._stream()
        self.lib.pack_erasures_matrix(plan, G, *(A.ptr(n) for n in ("hdr", "present", "meta", "fec_size",
                                                                    "parity_present")), E, A.ptr("packed"), st)
        self.pack_path = int(self.lib.lib.rfec_last_path())
        self.lib.recover_packed_matrix_out(plan, G, stride, capacity, A.ptr("shards"), A.ptr("parity"),
                                           A.ptr("packed"), A.ptr("recovered"), E, A.ptr("out_shards"),
                                           A.ptr("out_hdr"), A.ptr("out_index"), st)
        self.last_path = int(self.lib.lib.rfec_last_path())
        self._finish(A, "recover_packed_matrix")
        return (A.get("out_shards", np.uint8, (G, E, stride)), A.get("out_hdr", HDR_DTYPE, (G, E)),
                A.get("out_index", np.uint8, (G, E)), A.get("recovered", np.uint64, (G, 2)),
                A.get("packed", np.uint8, (G, pks)))


class GpuWire(wc.WireEngine):
    """The wire codec (rfec_wire_frame_fec / _seg, rfec_wire_parse and rfec_launch_wire_parse_split) on numpy
    inputs, every call's buffers in one guarded arena (wire_cases.WireEngine: each pointer at exactly its documented
    alignment, the outputs between canary guards, the inputs compared with what was uploaded).  last_path:
    rfec_wire_last_path's tag of the call (kernel id | grid blocks << 8, rfec_internal.h)."""

    has_tag = True

    def __init__(self, video_size=1000, device="cuda:0", tuning=0):
        import aux_kernel_cases as ac
        self.lib = native(video_size)
        self.c = ac.bind_launches(self.lib.lib)
        self.c.rfec_wire_last_path.restype, self.c.rfec_wire_last_path.argtypes = C.c_uint32, []
        self.c.rfec_wire_set_grid_cap.restype, self.c.rfec_wire_set_grid_cap.argtypes = None, [C.c_uint32]
        self.device = torch.device(device)
        self.be = TorchBackend(self.device)
        self.tuning = tuning  # RFEC_TUNE_WAVE_PARSE: the wave-per-datagram parse

    def set_grid_cap(self, blocks):
        """rfec_wire_set_grid_cap: process-global; the caller restores 0 in a finally."""
        self.c.rfec_wire_set_grid_cap(blocks)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def _ran(self):
        self.last_path = int(self.c.rfec_wire_last_path())

    @staticmethod
    def _opt(A, name):
        return A.ptr(name) if name in A.bufs else None

    def _frame_fec(self, A, N, stride, capacity, dstride):
        self.lib.wire_frame_fec(N, stride, capacity, A.ptr("parity"), A.ptr("meta"), A.ptr("fec_size"),
                                self._opt(A, "status"), A.ptr("stamps"), dstride, A.ptr("dgram"), A.ptr("dlen"),
                                self._stream(), order=self._opt(A, "order"))
        self._ran()

    def _frame_seg(self, A, N, stride, capacity, dstride):
        self.lib.wire_frame_seg(N, stride, capacity, A.ptr("shards"), A.ptr("hdr"), A.ptr("stamps"), dstride,
                                A.ptr("dgram"), A.ptr("dlen"), self._stream(), order=self._opt(A, "order"))
        self._ran()

    def _parse(self, A, N, dstride, stride, capacity, T, max_len, tuning):
        self.lib.set_tuning(self.tuning if tuning is None else tuning)
        try:
            if T is None:
                self.lib.wire_parse(N, dstride, A.ptr("dgram"), A.ptr("dlen"), stride, capacity, A.ptr("recs"),
                                    A.ptr("payload"), self._stream())
            else:
                rc = self.c.rfec_launch_wire_parse_split(N, dstride, A.ptr("dgram"), A.ptr("dlen"), stride, capacity,
                                                         A.ptr("recs"), A.ptr("payload"), max_len, A.ptr("split"), T,
                                                         self._stream())
                assert rc == 0, ("rfec_launch_wire_parse_split", rc)
            self._ran()
        finally:
            self.lib.set_tuning(0)


class GpuAux:
    """The helper kernels' launch shims (rfec_launch_*, razor_amd/csrc/rfec_internal.h) on numpy inputs: the
    engine of aux_kernel_cases.py.  pinned: rx_stage reads its map and its table source from rfec_pinned_alloc
    memory, as the receiver session passes them, instead of device memory."""

    def __init__(self, video_size=1200, device="cuda:0", pinned=False):
        import aux_kernel_cases as ac
        self.ac = ac
        self.lib = native(video_size)
        self.c = ac.bind_launches(self.lib.lib)
        # the runtime the library itself is linked to (found through its handle: one runtime per process)
        self.c.hipHostGetDevicePointer.restype = C.c_int
        self.c.hipHostGetDevicePointer.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint]
        self.device = torch.device(device)
        self.pinned = pinned
        self.wire = None  # parse_split's engine

    def _canary(self, nbytes):
        return torch.full((nbytes,), self.ac.CANARY, dtype=torch.uint8, device=self.device)

    def _run(self, fn, *args):
        rc = fn(*args, torch.cuda.current_stream(self.device).cuda_stream)
        assert rc == 0, (fn.__name__, rc)
        torch.cuda.synchronize(self.device)

    def _pinned(self, a):
        """`a` in an rfec_pinned_alloc block: (the block's keeper, the address the device reads it at -- the
        block's device pointer, from which rfec_pinned_alloc registers the offset the library adds)."""
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        arr, keep = self.lib.pinned_array((max(len(a), 16),), np.uint8)
        arr[:len(a)] = a
        d = C.c_void_p()
        assert self.c.hipHostGetDevicePointer(C.byref(d), arr.ctypes.data, 0) == 0 and d.value
        return keep, d.value

    def rx_split(self, recs, T):
        n = len(recs)
        d_r = _dev(recs, self.device)
        d_o = self._canary((n + self.ac.GUARD) * 8)
        self._run(self.c.rfec_launch_rx_split, d_r.data_ptr(), n, T, d_o.data_ptr())
        return _host(d_o, self.ac.SPLIT_DTYPE, (n + self.ac.GUARD,))

    def gather_rows(self, src, map_, stride):
        rows = len(map_)
        d_s, d_m = _dev(src, self.device), _dev(np.ascontiguousarray(map_, np.int32), self.device)
        d_o = self._canary((rows + self.ac.GUARD) * stride)
        self._run(self.c.rfec_launch_gather_rows, d_o.data_ptr(), d_s.data_ptr(), d_m.data_ptr(), rows, stride)
        return _host(d_o, np.uint8, (rows + self.ac.GUARD, stride))

    def rx_stage(self, src, map_, stride, tables):
        rows, tb = len(map_), len(tables)
        map_ = np.ascontiguousarray(map_, np.int32)
        d_s = _dev(src, self.device)
        if self.pinned:
            k_m, p_m = self._pinned(map_)
            k_t, p_t = self._pinned(tables)
        else:
            k_m = torch.zeros(4, dtype=torch.uint8, device=self.device) if rows == 0 else _dev(map_, self.device)
            k_t = torch.zeros(16, dtype=torch.uint8, device=self.device) if tb == 0 else _dev(tables, self.device)
            p_m, p_t = k_m.data_ptr(), k_t.data_ptr()
        d_o = self._canary((rows + self.ac.GUARD) * stride)
        d_t = self._canary(tb + self.ac.GUARD * 16)
        self._run(self.c.rfec_launch_rx_stage, d_o.data_ptr(), d_s.data_ptr(), p_m, rows, stride, d_t.data_ptr(), p_t,
                  tb)
        del k_m, k_t
        return _host(d_o, np.uint8, (rows + self.ac.GUARD, stride)), _host(d_t, np.uint8, (tb + self.ac.GUARD * 16,))

    def line_jobs(self, jobs, members, rows, outrows, stride):
        d_j, d_m = _dev(jobs, self.device), _dev(np.ascontiguousarray(members, np.int32), self.device)
        d_r, d_o = _dev(rows, self.device), _dev(outrows, self.device)
        self._run(self.c.rfec_launch_line_jobs, d_j.data_ptr(), len(jobs), d_m.data_ptr(), d_r.data_ptr(),
                  d_o.data_ptr(), stride)
        return _host(d_o, np.uint8, outrows.shape)

    def send_gather(self, blob, offsets, sizes, stride):
        """The blob in one rfec_pinned_alloc block; src: the addresses the sender passes for such a block
        (rfec_sender.c sd_stage: the host address + the block's device offset), 0 for a zero slot."""
        slots = len(offsets)
        keep, base = self._pinned(blob)
        assert base % 16 == 0
        src = np.where(offsets >= 0, base + offsets, 0).astype(np.uint64)
        d_s, d_z = _dev(src, self.device), _dev(np.ascontiguousarray(sizes, np.uint16), self.device)
        d_o = self._canary((slots + self.ac.GUARD) * stride)
        self._run(self.c.rfec_launch_send_gather, d_s.data_ptr(), d_z.data_ptr(), slots, stride, d_o.data_ptr())
        del keep
        return _host(d_o, np.uint8, (slots + self.ac.GUARD, stride))

    def parse_split(self, dgram, dlen, stride, capacity, max_len, T, tuning=0):
        """rfec_launch_wire_parse_split through GpuWire's guarded arena: (recs, payload, split entries + GUARD),
        the split buffer pre-filled with 0xAB."""
        if self.wire is None:
            self.wire = GpuWire(self.lib.video_size, self.device)
        return self.wire.parse_split(dgram, dlen, stride, capacity, max_len, T, tuning, tail=self.ac.GUARD)
