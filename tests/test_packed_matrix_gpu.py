"""GPU: rfec_pack_erasures_matrix + rfec_recover_packed_matrix_out (packed
matrix records, the sender's full row + column plans of k = 6..16) against
rfec_recover_batch_out on the same batch, bit for bit, and against the
reference receiver's erasure fixtures."""
import numpy as np
import pytest

import geometry_cases as gc
import packed_matrix_cases as pm
import parity_cases as pc
import pyoracle as po

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in po.manifest()["cases"]}


class PackedMatrixEngine:
    """gpu_engine.GpuEngine plus the packed matrix calls on numpy inputs."""

    def __init__(self, video_size=1000):
        from gpu_engine import GpuEngine
        self.eng = GpuEngine(video_size)
        self.lib, self.device = self.eng.lib, self.eng.device

    def encode(self, *a):
        return self.eng.encode(*a)

    def recover_out(self, *a):
        return self.eng.recover_out(*a)

    def recover_packed_matrix(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity, per_group,
                              packed=None):
        """rfec_pack_erasures_matrix (on the device, unless `packed` gives the
        records) then rfec_recover_packed_matrix_out: returns (out_shards,
        out_hdr, out_index, recovered, records [G][stride] as built).  The
        record buffer starts as 0x77, the outputs as 0x3C; the shards must come
        back untouched."""
        from gpu_engine import _dev, _host
        from razor_amd.fec import HDR_DTYPE
        G, k, stride = shards.shape
        E = per_group
        pks = self.lib.packed_matrix_stride(plan, E)
        assert pks > 0 and pks % 64 == 0
        st = torch.cuda.current_stream(self.device).cuda_stream
        d_sh = _dev(shards, self.device)
        d_p = _dev(parity, self.device)
        if packed is None:
            d_h = _dev(hdr, self.device)
            d_pr = _dev(np.ascontiguousarray(present, np.uint64), self.device)
            d_m = _dev(meta, self.device)
            d_f = _dev(np.ascontiguousarray(fsize, np.uint16), self.device)
            d_pp = _dev(np.ascontiguousarray(pp, np.uint64), self.device)
            d_pk = torch.full((G * pks,), 0x77, dtype=torch.uint8, device=self.device)
            self.lib.pack_erasures_matrix(plan, G, d_h.data_ptr(), d_pr.data_ptr(), d_m.data_ptr(), d_f.data_ptr(),
                                          d_pp.data_ptr(), E, d_pk.data_ptr(), st)
            self.pack_path = int(self.lib.lib.rfec_last_path())
            assert self.pack_path == gc.tag("PACK_MATRIX"), gc.tag_name(self.pack_path)
        else:
            assert packed.shape == (G, pks)
            d_pk = _dev(packed, self.device)
        d_rec = torch.full((G * 16,), 0xEE, dtype=torch.uint8, device=self.device)
        o_sh = torch.full((G * E * stride,), 0x3C, dtype=torch.uint8, device=self.device)
        o_h = torch.full((G * E * 20,), 0x3C, dtype=torch.uint8, device=self.device)
        o_i = torch.full((G * E,), 0x3C, dtype=torch.uint8, device=self.device)
        self.lib.recover_packed_matrix_out(plan, G, stride, capacity, d_sh.data_ptr(), d_p.data_ptr(),
                                           d_pk.data_ptr(), d_rec.data_ptr(), E, o_sh.data_ptr(), o_h.data_ptr(),
                                           o_i.data_ptr(), st)
        self.last_path = int(self.lib.lib.rfec_last_path())  # the dispatch tag: the kernel compiled for this k
        assert self.last_path == gc.tag("MATRIX_PACKED", plan.k), gc.tag_name(self.last_path)
        torch.cuda.synchronize(self.device)
        assert np.array_equal(_host(d_sh, np.uint8, (G, k, stride)), shards), "shards written"
        return (_host(o_sh, np.uint8, (G, E, stride)), _host(o_h, HDR_DTYPE, (G, E)), _host(o_i, np.uint8, (G, E)),
                _host(d_rec, np.uint64, (G, 2)), _host(d_pk, np.uint8, (G, pks)))


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    return PackedMatrixEngine


def _parity(eng, batch, E, where, min_slots=1):
    """Both decodes on one batch and per_group: the device-built records equal
    the host restatement's, and the decode from either gives
    rfec_recover_batch_out's results.  Returns rfec_recover_batch_out's."""
    plan, rx, rh, present, parity, meta, fs, pp, cap = batch
    cd16 = (cap + 15) // 16 * 16
    w_s, w_h, w_i, w_rec = eng.recover_out(plan, rx, rh, present, parity, meta, fs, pp, cap, E)
    host_pk = pm.pack_matrix_np(plan, rh, present, meta, fs, pp, E)
    sel = w_i != 0xFF
    assert sel.sum() >= min_slots, where
    for packed in (None, host_pk):
        g_s, g_h, g_i, g_rec, pk = eng.recover_packed_matrix(plan, rx, rh, present, parity, meta, fs, pp, cap, E,
                                                              packed=packed)
        assert np.array_equal(pk, host_pk), f"{where}: packed records"
        assert np.array_equal(g_i, w_i), f"{where}: out_index"
        assert np.array_equal(g_rec, w_rec), f"{where}: recovered"
        assert np.array_equal(g_h[sel], w_h[sel]), f"{where}: recovered headers"
        assert np.array_equal(g_s[sel][:, :cd16], w_s[sel][:, :cd16]), f"{where}: payloads"
    return w_s, w_h, w_i, w_rec


@pytest.mark.parametrize("k,S", pm.SHAPES)
def test_packed_matrix_decode_gpu(gpu, oracle1000, oracle1200, k, S):
    """0..6 erasures per group, lost parities and header rejections, per_group
    1, 2, 3 and k: records, out_index, recovered, the recovered headers and
    every payload chunk of a recovered slot, with the census of what the batch
    exercises taken on rfec_recover_batch_out's own results."""
    o = oracle1200 if S > 1000 else oracle1000
    batch = pm.lossy_matrix_rx(o, k, S, pm.G_CASES, pm.seed_of(k, S))
    plan, _, _, present, _, _, _, pp, _ = batch
    eng = gpu(o.video_size)
    for E in sorted({1, 2, 3, k}):
        w = _parity(eng, batch, E, f"k={k} S={S} E={E}", min_slots=pm.G_CASES // 4 if E > 1 else 1)
        c = pm.coverage(plan, present, pp, w[3], E)
        print(f"k={k} S={S} E={E}: {c}")
        pm.check_coverage(c, k, E)


def _clean_rx(o, k, S, G, lost, ragged=True):
    """A batch with segments lost[g] of every group erased (0xA5 payloads and
    header records) and every parity received."""
    col, rows = pm.shape_of(k)
    plan = o.plan_matrix(k, rows, col, 3)
    shards, hdr = o.fill_groups(3, G, k, S, ragged=ragged)
    cap = min(o.video_size, S)
    parity, meta, fsize, _ = o.encode_batch(plan, shards, hdr, cap)
    lost = np.asarray(lost, np.int64).reshape(G, -1)
    gi = np.arange(G)
    present = np.zeros((G, 2), np.uint64)
    rx, rh = shards.copy(), hdr.copy()
    m = np.full(G, (1 << k) - 1, np.int64)
    for c in range(lost.shape[1]):
        m &= ~(1 << lost[:, c])
        rx[gi, lost[:, c]] = 0xA5
        rh.view(np.uint8).reshape(G, k, 20)[gi, lost[:, c]] = 0xA5
    present[:, 0] = m
    pp = np.full(G, (1 << plan.n_lines) - 1, np.uint64)
    return shards, (plan, rx, rh, present, parity, meta, fsize, pp, cap)


def test_packed_matrix_one_group_gpu(gpu, oracle1000):
    """One group: segments 5 and 6 lost (one row, so both come back through
    their columns), per_group 1, 2 and k."""
    _, batch = _clean_rx(oracle1000, 10, 64, 1, [[5, 6]])
    for E in (1, 2, 10):
        w = _parity(gpu(), batch, E, f"G=1 E={E}")
        assert list(w[2][0, :min(E, 2)]) == [5, 6][:E]


def test_packed_matrix_partial_block_gpu(gpu, oracle1000):
    """37 groups: not a multiple of the checker's 16 groups per wave, a partial
    last block."""
    batch = pm.lossy_matrix_rx(oracle1000, 10, 64, 37, 44)
    for E in (1, 2, 10):
        _parity(gpu(), batch, E, f"G=37 E={E}")


def test_packed_matrix_c3full_shape_gpu(gpu, oracle1200):
    """k = 10, 1,200-byte slots at capacity 1,200 (the 1,200-byte library)."""
    batch = pm.lossy_matrix_rx(oracle1200, 10, 1200, 64, 5)
    assert batch[8] == 1200 and batch[1].shape[2] == 1200
    _parity(gpu(1200), batch, 2, "S=1200 cap=1200")


def test_packed_matrix_nothing_to_recover_gpu(gpu, oracle1000):
    """Every parity lost: nothing recovered, every out_index 0xFF; and a batch
    without erasures."""
    plan, rx, rh, present, parity, meta, fs, pp, cap = pm.lossy_matrix_rx(oracle1000, 10, 64, 100, 11)
    eng = gpu()
    for E in (2, 10):
        w = _parity(eng, (plan, rx, rh, present, parity, meta, fs, np.zeros_like(pp), cap), E, "no parity", 0)
        assert (w[2] == 0xFF).all() and not w[3].any()
    full = present.copy()
    full[:, 0] = (1 << 10) - 1
    shards, hdr = oracle1000.fill_groups(53, 100, 10, 64, ragged=True)
    w = _parity(eng, (plan, shards, hdr, full, parity, meta, fs, pp, cap), 2, "no erasures", 0)
    assert (w[2] == 0xFF).all() and not w[3].any()


class PackedMatrixAsInPlace(pc.DenseAsInPlace):
    """parity_cases.DenseAsInPlace through the packed matrix records
    (per_group = k, the out slots scattered back into the received layout)."""

    def recover(self, plan, shards, hdr, present, parity, meta, fsize, pp, capacity):
        G, k = shards.shape[:2]
        o_s, o_h, o_i, rec, _ = self.engine.recover_packed_matrix(plan, shards, hdr, present, parity, meta, fsize,
                                                                  pp, capacity, k)
        out_s, out_h = shards.copy(), hdr.copy()
        g, e = np.nonzero(o_i != 0xFF)
        out_s[g, o_i[g, e]] = o_s[g, e]
        out_h[g, o_i[g, e]] = o_h[g, e]
        return out_s, out_h, rec


@pytest.mark.parametrize("name", ["k10_full_le3", "k10_full_ragged_le4"])
def test_erasure_fixture_packed_matrix_gpu(gpu, oracle1000, name):
    """The reference receiver's verdicts and segment hashes (era_*.bin) of the
    full 3x4 plan through the packed matrix records."""
    pc.check_erasure_case(PackedMatrixAsInPlace(gpu()), oracle1000, CASES[name])


def test_packed_matrix_full_size_gpu(gpu, oracle1200):
    """8,192 groups of k = 10 at 1,200 B, two erasures each (the benchmark's
    c3full decode shape, enough blocks to cross the XCD rounds): every output
    of the packed decode equals rfec_recover_batch_out's."""
    o, G, k, S = oracle1200, 8192, 10, 1200
    rng = np.random.default_rng(20)
    lost = np.stack([rng.choice(k, 2, replace=False) for _ in range(G)])
    shards, (plan, rx, rh, present, parity, meta, fsize, pp, _) = _clean_rx(o, k, S, G, lost, ragged=False)
    gi = np.arange(G)
    eng = gpu(1200)
    w_s, w_h, w_i, w_rec = eng.recover_out(plan, rx, rh, present, parity, meta, fsize, pp, S, 2)
    g_s, g_h, g_i, g_rec, _ = eng.recover_packed_matrix(plan, rx, rh, present, parity, meta, fsize, pp, S, 2)
    sel = w_i != 0xFF
    assert sel.sum() > G  # most pairs are recoverable
    assert np.array_equal(g_i, w_i) and np.array_equal(g_rec, w_rec)
    assert np.array_equal(g_h[sel], w_h[sel]) and np.array_equal(g_s[sel], w_s[sel])
    assert np.array_equal(g_s[sel][:, :S], shards[gi[:, None], np.sort(lost, axis=1)][sel][:, :S])
