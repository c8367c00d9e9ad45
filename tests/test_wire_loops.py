"""The wire kernels' persistent-grid loops (wire_loop_cases.py): every case through the oracle in a guarded arena
(CPU), the conditions that keep a deep case from passing vacuously (CPU, on the oracle's records alone), and on the
GPU every case under rfec_wire_set_grid_cap with the kernel, the grid and the depth asserted from
rfec_wire_last_path; then each quarter-wave kernel once on the real grid, deep enough for a second header batch."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import pyoracle as po
import wire_cases as wc
import wire_loop_cases as wl


# -- CPU -----------------------------------------------------------------------------------------------------------
def test_wire_loop_case_set():
    """The case set holds what it is meant to: every N of the two lists at one geometry per kernel, every geometry
    at two deep N, the capped-at-3 N, and for each deep N the batches it claims by arithmetic."""
    by = {}
    for c in wl.CASES:
        by.setdefault(c.kernel, []).append(c)
    assert set(by) == set(wl.KERNELS)
    for kern, cs in by.items():
        quarter = wl.KERNELS[kern][2] == 4
        geoms = wl.Q_GEOMS if quarter else wl.W_GEOMS[kern]
        first = {(c.N, c.cap) for c in cs if c.geom == geoms[0]}
        assert first == {(n, 1) for n in (wl.Q_N1 if quarter else wl.W_N1)} | {(wl.Q_N3 if quarter else wl.W_N3, 3)}
        for g in geoms[1:]:
            assert sum(1 for c in cs if c.geom == g and wl.is_deep(c)) == 2, (kern, g)
        for c in cs:
            steps, batches = wl.depth(c)
            if wl.is_deep(c):
                assert batches == wl.CLAIM[(c.N, c.cap)] >= 2 and steps > wl.KERNELS[kern][3], wl.case_id(c)
            else:
                assert batches == 1 or c.N == 1025, wl.case_id(c)
    assert wl.Q_N1[-2:] == [1091, 2114] and wl.Q_N3 == 3265 and wl.W_N3 == 3125 and wl.W_N1[-1] == 2071
    # 1,024 datagrams at cap 1: every wave ends exactly at its batch's end; one more opens a second batch
    assert wl.depth(wl.Case("parse_q", wl.Q_GEOMS[0], 1024, 1)) == (16, 1)
    assert wl.depth(wl.Case("parse_q", wl.Q_GEOMS[0], 1025, 1)) == (17, 2)
    assert wl.depth(wl.Case("parse20", wl.Q_GEOMS[0], 1024, 1)) == (64, 1)
    assert wl.depth(wl.Case("parse20", wl.Q_GEOMS[0], 1025, 1)) == (65, 2)
    # the rotation of three buffers: wave 0's last step index mod 3 over the three N, the other waves' one less
    assert [((n - 1) // 16) % 3 for n in (1057, 1073, 1089)] == [0, 1, 2]


DEEP = [c for c in wl.CASES if wl.is_deep(c)]


@pytest.mark.parametrize("c", DEEP, ids=wl.case_id)
def test_wire_loop_deep_case_meets_its_conditions(c):
    """Parse: statuses 0, 1, -1, -2, -3 all occur, more than half are 0, a CRC mismatch that is not its wave's last
    unit is followed in the same lanes of the same wave by an OK datagram with data, and a CRC mismatch lies in a
    wave's second batch.  Framing: a zero-length output is followed by a valid one in the same lanes of the same
    wave.  From the oracle's outputs alone."""
    cond = wl.conditions(c, wl.make_inputs(c))
    assert all(cond.values()), (wl.case_id(c), cond)


@pytest.mark.parametrize("c", wl.CASES, ids=wl.case_id)
def test_wire_loop_case_oracle(oracle1000, c):
    """Every case through the oracle behind the guarded arena: the CPU run of the engine, the comparisons and the
    permuted form."""
    wl.run_case(wc.OracleWire(oracle1000), c)


def _fused_oracle_engine(oracle, family):
    import wire_encode_cases as wec
    import wire_send_cases as wsc
    import wire_send_shapes_cases as wss
    return {"fec": wec.OracleFused, "send": wsc.OracleSend, "shapes": wss.OracleShapes}[family](oracle)


@pytest.mark.parametrize("name", sorted(wl.FUSED))
def test_wire_loop_fused_case_oracle(oracle1000, name):
    wl.run_fused(name, _fused_oracle_engine(oracle1000, wl.FUSED[name][0]))
    if wl.FUSED[name][0] != "fec":  # the plan with a line of two SIM_SEG header batches is in the case
        x = wl.fused_inputs(name)
        plans = [x.plan] if hasattr(x, "plan") else x.plans
        assert max(p.line[l].count for p in plans for l in range(p.n_lines)) > 16


# -- GPU -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gwire():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuWire
    return GpuWire()


@pytest.mark.gpu
@pytest.mark.parametrize("c", wl.CASES, ids=wl.case_id)
def test_wire_loop_gpu(gwire, c):
    """The case under its grid cap: the case's kernel on exactly `cap` blocks (from rfec_wire_last_path), the depth
    it claims, and whole slots, whole records, split entries and lengths == the oracle's, in the guarded arena."""
    wl.run_case(gwire, c)
    assert gwire.last_path >> 8 == c.cap


@pytest.mark.gpu
def test_wire_grid_cap_is_off_by_default_gpu(gwire):
    """Without a cap a batch gets the blocks it needs (here 5 of 16 waves for 65 quads), and the cap at 0 again
    after a capped launch."""
    c = wl.Case("seg_q", wl.Q_GEOMS[4], 4 * 65, 1)
    x = wl.make_inputs(c)
    capacity, stride, dstride = c.geom
    for cap, blocks in ((0, 5), (2, 2), (0, 5)):
        gwire.set_grid_cap(cap)
        try:
            g, gl = gwire.frame_seg(x.data, x.hdr, x.stamps, capacity, dstride)
        finally:
            gwire.set_grid_cap(0)
        assert gwire.last_path == (wl.K_FRAME_SEG_Q | blocks << 8), hex(gwire.last_path)
        wl.same_frames(g, gl, x.dgram, x.dlen, f"cap {cap}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wl.FUSED))
def test_wire_loop_fused_gpu(gwire, name):
    """The fused kernel's case at one block: its kernel, grid 1 and more units than 16 waves from the tag; whole
    slots and lengths == the oracle composed, in the family's guarded arena."""
    import wire_encode_cases as wec
    import wire_send_cases as wsc
    import wire_send_shapes_cases as wss
    family = wl.FUSED[name][0]
    eng = {"fec": wec.GpuFused, "send": wsc.GpuSend, "shapes": wss.GpuShapes}[family](gwire.lib)
    wl.run_fused(name, eng, last_path=lambda: int(gwire.c.rfec_wire_last_path()), set_grid_cap=gwire.set_grid_cap)


def _real_grid_inputs(N, seed):
    """N all-valid datagrams of geometry (15, 16, 64), SIM_SEG and SIM_FEC by halves in random order."""
    o = po.Oracle(1000)
    capacity, stride, dstride = wl.Q_GEOMS[4]
    rng = np.random.default_rng(seed)
    h = N // 2
    data, hdr, sizes, stamps = wc.random_batch(rng, h, stride, capacity, seg=True)
    a, al = o.frame_seg_batch(data, hdr, stamps, capacity, dstride)
    data, hdr, sizes, stamps = wc.random_batch(rng, N - h, stride, capacity, seg=False)
    b, bl = o.frame_fec_batch(data, hdr, sizes, None, stamps, capacity, dstride)
    pick = rng.permutation(N)
    return np.concatenate([a, b])[pick], np.concatenate([al, bl])[pick], rng


def _resident(gwire, kid, run):
    """(blocks per CU, CUs): from the grid of a first launch that needs four blocks per CU."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    run(4 * 16 * cus * 4)
    assert gwire.last_path & 0xFF == kid
    grid = gwire.last_path >> 8
    assert grid % cus == 0 and 1 <= grid // cus < 4, (grid, cus)
    return grid // cus, cus


def _deep_n(cus, B):
    return 16 * 4 * 16 * cus * B + 4 * 16 * cus * B + 3


@pytest.mark.gpu
def test_wire_parse_real_grid_gpu(gwire, oracle1000):
    """k_parse_q on the grid it gets without a cap, with N past every wave's first header batch (grid x 16 waves x
    16 quads x 4 < N, from the tag): all-valid datagrams, 1 % with a flipped byte; records, payloads and split
    entries == the oracle's."""
    capacity, stride, dstride = wl.Q_GEOMS[4]
    gwire.tuning = 0

    def run(N, flip=False):
        dgram, dlen, rng = _real_grid_inputs(N, N)
        if flip:
            idx = np.nonzero(rng.random(N) < 0.01)[0]
            pos = (rng.random(len(idx)) * dlen[idx]).astype(np.int64)
            dgram[idx, pos] ^= (1 << rng.integers(0, 8, len(idx))).astype(np.uint8)
        recs, pay, split = gwire.parse_split(dgram, dlen, stride, capacity, 0, 3)
        orecs, opay = oracle1000.parse_batch(dgram, dlen, stride, capacity)
        wl.same_parse(recs, pay, orecs, opay, f"k_parse_q N={N}")
        wl.same_split(split, orecs, 3, f"k_parse_q N={N}")
        return orecs

    B, cus = _resident(gwire, wl.K_PARSE_Q, run)
    N = _deep_n(cus, B)
    orecs = run(N, flip=True)
    grid = gwire.last_path >> 8
    assert gwire.last_path & 0xFF == wl.K_PARSE_Q and grid == cus * B and grid * 16 * 16 * 4 < N, (grid, N)
    bad = int((orecs["status"] == -1).sum())
    assert N // 200 < bad < N // 50 and int((orecs["status"] == 0).sum()) == N - bad


@pytest.mark.gpu
@pytest.mark.parametrize("seg", [True, False], ids=["seg", "fec"])
def test_wire_frame_real_grid_gpu(gwire, oracle1000, seg):
    """k_frame_seg_q / k_frame_fec_q on the grid they get without a cap, with N past every wave's 16th quad (from
    the tag): whole slots and lengths == the oracle's."""
    capacity, stride, dstride = wl.Q_GEOMS[4]
    kid = wl.K_FRAME_SEG_Q if seg else wl.K_FRAME_FEC_Q

    def run(N):
        rng = np.random.default_rng(N + seg)
        data, hdr, sizes, stamps = wc.random_batch(rng, N, stride, capacity, seg=seg)
        if seg:
            g, gl = gwire.frame_seg(data, hdr, stamps, capacity, dstride)
            o, ol = oracle1000.frame_seg_batch(data, hdr, stamps, capacity, dstride)
        else:
            g, gl = gwire.frame_fec(data, hdr, sizes, None, stamps, capacity, dstride)
            o, ol = oracle1000.frame_fec_batch(data, hdr, sizes, None, stamps, capacity, dstride)
        wl.same_frames(g, gl, o, ol, f"N={N}")

    B, cus = _resident(gwire, kid, run)
    N = _deep_n(cus, B)
    run(N)
    grid = gwire.last_path >> 8
    assert gwire.last_path & 0xFF == kid and grid == cus * B and grid * 16 * 16 * 4 < N, (grid, N)
