"""CPU: the packed matrix records' geometry and argument checks (no launch),
the host restatement of their layout, and a census of the batches the GPU
parity test runs on (cascades, schedules of more than four steps, rejected
lines), taken with the oracle."""
import numpy as np
import pytest

import packed_matrix_cases as pm
import pyoracle as po


def test_packed_matrix_geometry(product):
    """rfec_packed_matrix_stride and the two calls' checks: the sender's full
    row + column plans of k = 6..16 only, per_group in [1, k]."""
    from razor_amd.fec import RfecError
    full10 = product.plan_matrix(10, 3, 4, 3)
    assert product.packed_matrix_stride(full10, 1) == 192  # 16 + 148
    assert product.packed_matrix_stride(full10, 2) == 320  # 16 + 2 x 148 = 312
    for k, E in ((6, 6), (13, 3), (16, 16)):
        col, rows = pm.shape_of(k)
        S = 24 + 20 * (col - 1) + 24 + 20 * (rows - 1)
        plan = product.plan_matrix(k, rows, col, 3)
        assert product.packed_matrix_stride(plan, E) == (16 + E * S + 63) // 64 * 64 == pm.stride_of(k, E)
    for k in range(6, 17):  # the plans the sender picks at small k are all covered
        assert product.packed_matrix_stride(product.plan_from_fraction(k, 80, 3), 1) == pm.stride_of(k, 1), k
    refused = [(product.plan_matrix(10, 3, 4, 1), 2),    # rows only
               (product.plan_matrix(10, 3, 4, 2), 2),    # columns only
               (product.plan_matrix(12, 6, 2, 3), 2),    # rows of 2
               (product.plan_from_fraction(5, 80, 3), 2),  # strip mode
               (product.plan_from_fraction(17, 80, 3), 2),
               (full10, 0), (full10, 11)]
    for plan, E in refused:
        assert product.packed_matrix_stride(plan, E) == 0, (plan, E)
        with pytest.raises(RfecError):
            product.pack_erasures_matrix(plan, 4, 16, 16, 16, 16, 16, E, 16)
        with pytest.raises(RfecError):
            product.recover_packed_matrix_out(plan, 4, 1200, 1200, 16, 16, 16, 16, E, 16, 16, 16)
    with pytest.raises(RfecError):  # records not 16-byte aligned
        product.recover_packed_matrix_out(full10, 4, 1200, 1200, 16, 16, 24, 16, 2, 16, 16, 16)
    with pytest.raises(RfecError):
        product.pack_erasures_matrix(full10, 4, 16, 16, 16, 16, 16, 2, 24)
    with pytest.raises(RfecError):  # NULL buffers
        product.recover_packed_matrix_out(full10, 4, 1200, 1200, None, None, 16, None, 2, None, None, None)
    with pytest.raises(RfecError):
        product.pack_erasures_matrix(full10, 4, None, None, None, None, None, 2, 16)
    with pytest.raises(RfecError):  # NULL records
        product.pack_erasures_matrix(full10, 4, 16, 16, 16, 16, 16, 2, None)
    with pytest.raises(RfecError):  # groups x slots beyond 32 bits
        product.pack_erasures_matrix(full10, 1 << 29, 16, 16, 16, 16, 16, 10, 16)
    with pytest.raises(RfecError):  # stride not a multiple of 16 (check_geometry)
        product.recover_packed_matrix_out(full10, 4, 1000, 1000, 16, 16, 16, 16, 2, 16, 16, 16)
    # no groups: nothing to do, no buffer needed
    product.pack_erasures_matrix(full10, 0, None, None, None, None, None, 2, None)
    product.recover_packed_matrix_out(full10, 0, 1200, 1200, None, None, None, None, 2, None, None, None)
    # the row-layout records keep refusing these plans
    assert product.packed_stride(full10, 2) == 0


def _group(k, lost):
    col, rows = pm.shape_of(k)
    nr = rows if k - (rows - 1) * col >= 2 else rows - 1
    n = nr + col
    hdr = np.zeros((1, k), po.HDR_DTYPE)
    hdr["seq"] = np.arange(100, 100 + k)
    hdr["size"] = 40
    hdr[0, lost:lost + 1].view(np.uint8)[...] = 0xA5  # an erased record: whatever the array held
    meta = np.zeros((1, n), po.HDR_DTYPE)
    meta["seq"] = np.arange(7, 7 + n)
    fs = (300 + np.arange(n)).astype(np.uint16)[None, :]
    present = np.array([[((1 << k) - 1) & ~(1 << lost), 0]], np.uint64)
    pp = np.array([(1 << n) - 1], np.uint64)
    return hdr, meta, fs, present, pp


def _seqs(rec, o, n):
    return [int(rec[o + 20 * q:o + 20 * q + 20].view(po.HDR_DTYPE)[0]["seq"]) for q in range(n)]


def test_packed_matrix_layout(oracle1000):
    """pack_matrix_np (what the GPU tests compare rfec_pack_erasures_matrix
    against) follows razor_fec.h's layout: k = 10 (3 rows of 4, 2 in the last),
    segment 5 lost, two slots."""
    k, E = 10, 2
    plan = oracle1000.plan_matrix(k, 3, 4, 3)
    hdr, meta, fs, present, pp = _group(k, 5)
    rec = pm.pack_matrix_np(plan, hdr, present, meta, fs, pp, E)
    assert rec.shape == (1, 320)
    rec = rec[0]
    u64 = rec[:16].view(np.uint64)
    assert u64[0] == present[0, 0] and u64[1] == 0x7F
    # slot 0 at +16: segment 5 = row 1 (line 1: 4 5 6 7), column 1 (line 3 + 1: 1 5 9)
    o = 16
    assert rec[o:o + 20].view(po.HDR_DTYPE)[0]["seq"] == meta[0, 1]["seq"]
    assert rec[o + 20:o + 22].view(np.uint16)[0] == fs[0, 1] and not rec[o + 22:o + 24].any()
    assert _seqs(rec, o + 24, 3) == [104, 106, 107]
    o = 16 + 84  # the column half: 24 + 2 x 20 = 64 bytes
    assert rec[o:o + 20].view(po.HDR_DTYPE)[0]["seq"] == meta[0, 4]["seq"]
    assert rec[o + 20:o + 22].view(np.uint16)[0] == fs[0, 4] and not rec[o + 22:o + 24].any()
    assert _seqs(rec, o + 24, 2) == [101, 109]
    assert not rec[16 + 148:].any()  # no second erasure: slot 1 and the padding are zeros
    # a second erasure in the same row: its position in slot 0's row half holds zeros, not the array's bytes
    present[0, 0] = int(present[0, 0]) & ~(1 << 7)
    hdr[0, 7:8].view(np.uint8)[...] = 0xA5
    rec = pm.pack_matrix_np(plan, hdr, present, meta, fs, pp, E)[0]
    assert _seqs(rec, 16 + 24, 3) == [104, 106, 0] and not rec[16 + 24 + 40:16 + 84].any()
    o = 16 + 148  # slot 1: segment 7 = row 1, column 3 (line 6: 3 7; past the line's end: zeros)
    assert _seqs(rec, o + 24, 3) == [104, 0, 106]
    assert rec[o + 84:o + 104].view(po.HDR_DTYPE)[0]["seq"] == meta[0, 6]["seq"]
    assert _seqs(rec, o + 84 + 24, 2) == [103, 0]
    assert not rec[16 + 2 * 148:].any()


def test_packed_matrix_layout_row_without_line(oracle1000):
    """k = 13: the last row has one member and no line, so the row half of
    segment 12's slot is zeros; its column half is line 3 + 0 (0 4 8 12)."""
    k = 13
    plan = oracle1000.plan_matrix(k, 4, 4, 3)
    assert plan.n_lines == 7
    hdr, meta, fs, present, pp = _group(k, 12)
    rec = pm.pack_matrix_np(plan, hdr, present, meta, fs, pp, 1)
    assert rec.shape == (1, pm.stride_of(13, 1)) and rec.shape[1] == 192  # 16 + 84 + 84
    rec = rec[0]
    assert not rec[16:16 + 84].any()
    o = 16 + 84
    assert rec[o:o + 20].view(po.HDR_DTYPE)[0]["seq"] == meta[0, 3]["seq"]
    assert rec[o + 20:o + 22].view(np.uint16)[0] == fs[0, 3]
    assert _seqs(rec, o + 24, 3) == [100, 104, 108]
    assert not rec[16 + 168:].any()


@pytest.mark.parametrize("k,S", pm.SHAPES)
def test_packed_matrix_inputs_reach_every_path(oracle1000, oracle1200, k, S):
    """The batches of the GPU parity test, against the oracle: enough groups
    that recover, clean cascades, rejected lines (alone and in cascades) and,
    for k >= 9, schedules of more than four steps (the serial path of the
    four-lane checker)."""
    o = oracle1200 if S > 1000 else oracle1000
    plan, rx, rh, present, parity, meta, fs, pp, cap = pm.lossy_matrix_rx(o, k, S, pm.G_CASES, pm.seed_of(k, S))
    for E in (k, 2):
        rec = o.recover_batch_out(plan, rx, rh, present, parity, meta, fs, pp, cap, E)[3]
        c = pm.coverage(plan, present, pp, rec, E)
        print(f"k={k} S={S} E={E}: {c}")
        pm.check_coverage(c, k, E)
