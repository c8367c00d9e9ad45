"""The geometry cases (geometry_cases.py) against the oracle behind guarded
arenas (CPU) and against the HIP kernels (GPU); the self-test that the guarded
arena and the full-slot comparison can fail; the decodes on both sides of the
buffer-descriptor bound."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import geometry_cases as gc
import guarded_arena as ga
import pyoracle as po

IDS = [c["id"] for c in gc.CASES]
_REACHED = {}  # case id -> the tags it asserted on the GPU


def _oracle_engine(o):
    return lambda tuning: ga.OracleArenaEngine(o)


@pytest.mark.parametrize("cid", IDS)
def test_geometry_oracle(oracle1000, cid):
    """Every case on the oracle behind the guarded arena: its inputs meet the
    share conditions (a quarter of the groups recover a segment; with header
    corruptions the exact peel differs from the mask-only peel in 5 % of them)
    and the oracle meets the slot contract the GPU run is held to."""
    c = gc.CASES[IDS.index(cid)]
    gc.run_case(_oracle_engine(oracle1000), oracle1000, c)


def test_case_table_names_every_tag():
    """The tags the cases name, with the pack launches of the packed cases, are the
    whole enum, and the enum restated in geometry_cases is rfec_internal.h's."""
    src = (Path(__file__).resolve().parent.parent / "razor_amd" / "csrc" / "rfec_internal.h").read_text()
    body = re.search(r"enum\s*\{\s*(RFEC_PATH_NONE\s*=\s*0\s*,[^}]*)\}", src).group(1)
    names = [re.fullmatch(r"RFEC_PATH_(\w+?)(\s*=\s*0)?", x.strip()).group(1) for x in body.split(",")]
    assert names == sorted(gc.KIND, key=gc.KIND.get) and list(gc.KIND.values()) == list(range(len(names)))
    flags = {n: int(v, 16) for n, v in re.findall(r"#define RFEC_PATH_(\w+) (0x[0-9a-fA-F]+)u", src)}
    assert flags == dict(SLOTS=gc.SLOTS, PACKED=gc.PACKED, FAST=gc.FAST, DENSE=gc.DENSE)
    assert {t & 0xFF for t in gc.ALL_TAGS} == set(gc.KIND.values()) - {gc.KIND["NONE"]}
    named = {c["tag"] for c in gc.CASES} | {gc.tag(f"PACK_{c['packed'].upper()}") for c in gc.CASES if c.get("packed")}
    assert named - gc.ALL_TAGS == set(), [gc.tag_name(t) for t in named - gc.ALL_TAGS]
    missing = gc.ALL_TAGS - named - set(gc.NOT_REACHED)
    assert not missing and not (set(gc.NOT_REACHED) & named), [gc.tag_name(t) for t in missing]
    assert all(len(r) > 20 for r in gc.NOT_REACHED.values())
    # and the sweep's group counts follow the rules as restated
    assert (gc.enc_gpb(10), gc.enc_gpb(16), gc.enc_gpb(34), gc.enc_gpb(36)) == (64, 48, 24, 20)
    assert (gc.peel_gpb(10, 7), gc.peel_gpb(36, 12), gc.fused_gpb(3), gc.fused_gpb(8)) == (64, 32, 64, 32)


def test_hdr_heavy_cases():
    """Every path whose grid holds header blocks has a case with more header
    than payload units (every == 0 by the launcher's rule, which run_case
    asserts for the case), or is listed in NO_HDR_HEAVY with the reason why no
    batch reaches that; the reason is checked over every group count up to 4096
    at the path's smallest capacity.  The worked values are the launchers' for
    257 groups of one chunk."""
    assert [gc.every_of(t, p, 257, 16, E) for t, p, E in (
        (gc.tag("ENC_ROWS", 10), gc.R10, 0), (gc.tag("ENC_ROWS", 32), gc.R32, 0),
        (gc.tag("ENC_ROWS_RT", 4), ("rows", 12, 4), 0), (gc.tag("ENC_MATRIX", 16), ("full", 16), 0),
        (gc.tag("ENC_ROWS_RT", 16), ("rows", 34, 16), 0), (gc.tag("MATRIX_DENSE", 10), ("full", 10), 1),
        (gc.tag("CASCADE_DENSE", 64), ("sub", 40), 1), (gc.tag("DEC_ROWS", 10 | gc.SLOTS | gc.PACKED), gc.R10, 1),
        (gc.tag("DEC_FLAT", 4), gc.R10, 0), (gc.tag("DEC_FLAT", 8), gc.C8, 2))] == [1, 1, 1, 2, 0, 1, 1, 1, 0, 0]
    heavy = {c["tag"] for c in gc.CASES if c.get("every") == 0 and gc.every_of_case(c) == 0}
    for t in sorted(gc.ALL_TAGS):
        shape = next(c for c in gc.CASES if c["tag"] == t) if any(c["tag"] == t for c in gc.CASES) else None
        if shape is None or gc.every_of_case(shape) is None:  # (the pack kernels; no header blocks in the grid)
            assert t not in heavy and t not in gc.NO_HDR_HEAVY
            continue
        assert (t in heavy) != (t in gc.NO_HDR_HEAVY), gc.tag_name(t)
        if t in gc.NO_HDR_HEAVY:
            why, plan, cap, Es = gc.NO_HDR_HEAVY[t]
            assert len(why) > 20
            assert min(gc.every_of(t, plan, G, cap, E) for G in range(1, 4097) for E in Es) >= 1, gc.tag_name(t)


def _gpu_engine(c):
    """GpuEngine behind its guarded arena; the packed matrix records have their
    engine in test_packed_matrix_gpu.py."""
    if c.get("packed") == "matrix":
        from test_packed_matrix_gpu import PackedMatrixEngine
        return lambda tuning: PackedMatrixEngine(1000)
    from gpu_engine import GpuEngine
    return lambda tuning: GpuEngine(1000, "cuda:0", tuning, random_workspace=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", IDS)
def test_geometry_gpu(oracle1000, cid):
    c = gc.CASES[IDS.index(cid)]
    _REACHED[cid] = gc.run_case(_gpu_engine(c), oracle1000, c)


@pytest.mark.gpu
def test_geometry_tags_complete_gpu():
    """The union of the tags the GPU cases asserted is the whole enum."""
    for c in gc.CASES:  # (a partial run: the cases it left out run here)
        if c["id"] not in _REACHED:
            _REACHED[c["id"]] = gc.run_case(_gpu_engine(c), po.Oracle(1000), c)
    reached = {t for ts in _REACHED.values() for t in ts}
    want = gc.ALL_TAGS - set(gc.NOT_REACHED)
    assert not gc.NOT_REACHED
    assert reached == want, ([gc.tag_name(t) for t in want - reached], [gc.tag_name(t) for t in reached - want])


# ---------------------------------------------------------------------------------------------------------------
# the harness must be able to fail
# ---------------------------------------------------------------------------------------------------------------
class _Mutated(ga.OracleArenaEngine):
    def __init__(self, o, fn):
        super().__init__(o)
        self.mutate = lambda A, what: fn(A)


ENC = dict(op="encode", id="self-encode", plan=("rows", 10, 4), G=5, cap=40, extra=16, tuning=0, E=0, tag=0, seed=5,
           corrupt=0.0)
REC = dict(ENC, op="recover", id="self-recover", G=40)
OUT = dict(REC, id="self-recover-out", E=2)


def _poke(A, name, off, v=None):
    view = A.view(name)
    view[off] = (int(view[off]) ^ 0x01) if v is None else v


def _guard(A, name, delta):
    b = A.bufs[name]
    A.mem[b.off + (b.nbytes if delta >= 0 else 0) + delta] ^= 0xFF


def _first_received(A, k=10):
    p = int(A.get("present", np.uint64, (-1, 2))[0, 0])
    return next(i for i in range(k) if (p >> i) & 1)


MUTATIONS = [
    # (case, mutation, the words the report must hold)
    ("guard-before-output", ENC, lambda A: _guard(A, "parity", -1), ["guard before parity", "1 bytes", "offset -1 "]),
    ("guard-after-output", ENC, lambda A: _guard(A, "parity", 0), ["guard after parity", "1 bytes", "offset 0 "]),
    ("guard-after-out-slot", OUT, lambda A: _guard(A, "out_shards", 15), ["guard after out_shards", "offset 15 "]),
    ("guard-before-workspace", REC, lambda A: _guard(A, "workspace", -16), ["guard before workspace", "offset -16 "]),
    ("input-encode-shards", ENC, lambda A: _poke(A, "shards", 77), ["input shards was written", "offset 77"]),
    ("input-encode-hdr", ENC, lambda A: _poke(A, "hdr", 3), ["input hdr was written", "offset 3"]),
    ("input-recover-parity", REC, lambda A: _poke(A, "parity", 9), ["input parity was written", "offset 9"]),
    ("input-recover-fec-size", REC, lambda A: _poke(A, "fec_size", 1), ["input fec_size was written"]),
    ("input-recover-present", REC, lambda A: _poke(A, "present", 0), ["input present was written"]),
    ("input-out-shards", OUT, lambda A: _poke(A, "shards", 5), ["input shards was written", "offset 5"]),
    ("received-segment", REC, lambda A: _poke(A, "shards", _first_received(A) * 64 + 63),
     ["a received segment of shards was written", "1 rows", "at byte 63"]),
    ("received-header", REC, lambda A: _poke(A, "hdr", _first_received(A) * 20 + 19),
     ["a received segment's header of hdr was written", "at byte 19"]),
    # the full-slot comparison: 16 CD = 48, the stride 64, every fec_data_size <= 40
    ("parity-past-L", ENC, lambda A: _poke(A, "parity", 47, 1), ["parity group 0 line 0", "16 CD = 48) are not zero"]),
    ("parity-tail", ENC, lambda A: _poke(A, "parity", 64 + 48, 0),
     ["parity group 0 line 1", "stride = 64) were written"]),
    ("out-slot-tail", OUT, lambda A: _poke(A, "out_shards", 63, 0), ["out_shards group 0 slot 0", "written"]),
]


@pytest.mark.parametrize("name", [m[0] for m in MUTATIONS])
def test_checks_can_fail(oracle1000, name):
    """One wrong byte, written into the arena after the oracle's call, must be
    reported under the right buffer name: in a guard before / after a buffer, in
    an input-only buffer, in a received segment or its header, past
    fec_data_size in a parity line, past the last chunk of a slot."""
    _, case, fn, words = next(m for m in MUTATIONS if m[0] == name)
    gc.run_case(_oracle_engine(oracle1000), oracle1000, case)  # the unmutated case passes
    with pytest.raises(AssertionError) as e:
        gc.run_case(lambda tuning: _Mutated(oracle1000, fn), oracle1000, case)
    msg = str(e.value)
    assert all(w in msg for w in words), (words, msg)


def test_arena_layout_is_minimally_aligned():
    """Every buffer starts at exactly its documented alignment (a multiple of it
    and of nothing larger) behind at least 4 KiB of canary on either side."""
    bufs = [ga.Buf(n, 100 + 3 * i, 0x5A, "out") for i, n in enumerate(ga.ALIGN)]
    A = ga.Arena(ga.NumpyBackend(), bufs)
    end = 0
    for b in bufs:
        p = A.ptr(b.name)
        assert p % b.align == 0 and p % (2 * b.align) != 0, b.name
        assert b.off - end >= ga.GUARD and (A.mem[end:b.off] == ga.CANARY).all()
        end = b.off + b.nbytes
    assert len(A.mem) - end >= ga.GUARD and (A.mem[end:] == ga.CANARY).all()
    A.check("untouched")


# ---------------------------------------------------------------------------------------------------------------
# the decodes on both sides of the buffer-descriptor bound
# ---------------------------------------------------------------------------------------------------------------
K_WAVE, K_NOLOAD = 64, 0x7FFFFFF0  # rfec_device.h kWave, kNoLoad
BOUND_K, BOUND_G, BOUND_CAP = 10, 66, 16


def _bound_strides(k, n_lines):
    """The largest multiple-of-16 stride with (kWave + 1) * max(k, n_lines) * stride < kNoLoad (the fused decodes'
    bound; the cascade's has k alone: the same for k >= n_lines) and the smallest that violates it."""
    per = (K_WAVE + 1) * max(k, n_lines)
    below = (K_NOLOAD - 1) // per // 16 * 16
    assert per * below < K_NOLOAD <= per * (below + 16)
    return below, below + 16


def test_recover_packed_stride_above_descriptor_bound(product):
    """rfec_recover_packed_out has no fallback kernel: a stride at which a wave's
    groups do not fit one buffer descriptor is RFEC_EINVAL, the largest one
    below is accepted by the same checks (no launch here: the records are NULL
    past them)."""
    from razor_amd.fec import RfecError
    plan = product.plan_matrix(BOUND_K, 3, 4, 1)
    below, above = _bound_strides(BOUND_K, 3)
    A = 1 << 20
    with pytest.raises(RfecError) as e:
        product.recover_packed_out(plan, BOUND_G, above, BOUND_CAP, A, A, A, A, 2, A, A, A)
    assert "(-1)" in str(e.value) and "too large" in str(e.value)
    with pytest.raises(RfecError) as e:  # below the bound the geometry passes: the next check (NULL buffers) speaks
        product.recover_packed_out(plan, BOUND_G, below, BOUND_CAP, None, A, A, A, 2, A, A, A)
    assert "NULL buffer" in str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["below", "above"])
@pytest.mark.parametrize("shape,output", [("rows", "in_place"), ("rows", "dense"), ("rows", "packed"),
                                          ("full", "in_place"), ("full", "dense")])
def test_recover_stride_at_descriptor_bound_gpu(product, oracle1000, shape, output, side):
    """Decodes whose stride is the largest the buffer descriptor of a wave's
    groups allows, and 16 bytes more: 66 groups of capacity 16 (one chunk a
    slot, so one wave of the flat form spans 64 groups and its last lanes' offsets
    reach the end of the descriptor's range).  Row plan: the fused decode below,
    the LDS peel + replay above; the sender's 3x4 plan: the cascade decode
    below, the peel + replay above; the packed records (row plan): decode
    below, RFEC_EINVAL above.  The batch (about 2.8 GB) is built on the device:
    zero slots with the compact batch in their first 16 bytes.  Results equal
    the oracle's on the compact layout."""
    import torch

    from razor_amd.fec import RfecError
    lib, o = product, oracle1000
    lib.lib.rfec_last_path.restype = C.c_uint32
    k, G, cap = BOUND_K, BOUND_G, BOUND_CAP
    c = dict(op="recover", id=f"bound-{shape}", plan=("rows", k, 4) if shape == "rows" else ("full", k), G=G, cap=cap,
             extra=0, tuning=0, E=0, tag=0, seed=66, corrupt=0.6, max_erase=4 if shape == "rows" else 5,
             events=1 if shape == "rows" else 3)
    plan, rx, rh, present, parity, meta, fs, pp, clean, e_s, e_h, e_rec = gc.build_rx(o, c)
    n = plan.n_lines
    below, above = _bound_strides(k, n)
    stride = below if side == "below" else above
    E = 0 if output == "in_place" else 2
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)

    sh = torch.zeros((G, k, stride), dtype=torch.uint8, device=dev)
    sh[:, :, :16] = up(rx).view(G, k, 16)
    par = torch.zeros((G, n, stride), dtype=torch.uint8, device=dev)
    par[:, :, :16] = up(parity).view(G, n, 16)
    d_h, d_pr, d_m, d_f, d_pp = up(rh), up(np.ascontiguousarray(present, np.uint64)), up(meta), up(
        np.ascontiguousarray(fs, np.uint16)), up(np.ascontiguousarray(pp, np.uint64))
    d_rec = torch.full((G * 16,), 0xEE, dtype=torch.uint8, device=dev)
    ws = torch.zeros((max(16, lib.workspace_size(plan, G)),), dtype=torch.uint8, device=dev)
    if E:
        o_s = torch.full((G, E, stride), 0x3C, dtype=torch.uint8, device=dev)
        o_h = torch.full((G * E * 20,), 0x3C, dtype=torch.uint8, device=dev)
        o_i = torch.full((G * E,), 0x3C, dtype=torch.uint8, device=dev)
    fused = gc.tag("DEC_FLAT", 4) if shape == "rows" else (gc.tag("MATRIX_DENSE", k) if E else gc.tag("CASCADE", 32))
    peel = gc.tag("PEEL_FLAT", 4 | gc.FAST | (gc.DENSE if E else 0))
    try:
        if output == "in_place":
            lib.recover_batch(plan, G, stride, cap, sh.data_ptr(), d_h.data_ptr(), d_pr.data_ptr(), par.data_ptr(),
                              d_m.data_ptr(), d_f.data_ptr(), d_pp.data_ptr(), d_rec.data_ptr(), ws.data_ptr(), st)
        elif output == "dense":
            lib.recover_batch_out(plan, G, stride, cap, sh.data_ptr(), d_h.data_ptr(), d_pr.data_ptr(), par.data_ptr(),
                                  d_m.data_ptr(), d_f.data_ptr(), d_pp.data_ptr(), d_rec.data_ptr(), E, o_s.data_ptr(),
                                  o_h.data_ptr(), o_i.data_ptr(), ws.data_ptr(), st)
        else:
            pk = torch.full((G * lib.packed_stride(plan, E),), 0x77, dtype=torch.uint8, device=dev)
            lib.pack_erasures(plan, G, d_h.data_ptr(), d_pr.data_ptr(), d_m.data_ptr(), d_f.data_ptr(), d_pp.data_ptr(),
                              E, pk.data_ptr(), st)
            args = (plan, G, stride, cap, sh.data_ptr(), par.data_ptr(), pk.data_ptr(), d_rec.data_ptr(), E,
                    o_s.data_ptr(), o_h.data_ptr(), o_i.data_ptr(), st)
            if side == "above":
                with pytest.raises(RfecError):
                    lib.recover_packed_out(*args)
                return
            lib.recover_packed_out(*args)
        path = int(lib.lib.rfec_last_path())
        torch.cuda.synchronize(dev)
        if output == "packed":
            assert path == gc.tag("DEC_ROWS", 10 | gc.SLOTS | gc.PACKED), gc.tag_name(path)
        else:
            assert path == (fused if side == "below" else peel), gc.tag_name(path)
        rec = d_rec.cpu().numpy().view(np.uint64).reshape(G, 2)
        if E == 0:
            assert np.array_equal(rec, e_rec)
            got_s = sh[:, :, :16].cpu().numpy()
            got_h = d_h.cpu().numpy().view(po.HDR_DTYPE).reshape(G, k)
            m = np.array([[(gc._w(rec, g) >> i) & 1 for i in range(k)] for g in range(G)], bool)
            assert m.sum() >= G // 4
            assert np.array_equal(got_h[m], e_h[m]) and np.array_equal(got_s[m], e_s[m])
            keep = ga.present_rows(present, k).reshape(G, k)
            assert np.array_equal(got_h[keep], rh[keep]) and np.array_equal(got_s[keep], rx[keep])
            assert not bool(sh[:, :, 16:4096].any()) and not bool(sh[:, :, stride - 4096:].any())
        else:
            x_s, x_h, x_i, x_rec = o.recover_batch_out(plan, rx, rh, present, parity, meta, fs, pp, cap, E)
            assert np.array_equal(rec, x_rec)
            assert np.array_equal(o_i.cpu().numpy().reshape(G, E), x_i)
            m = x_i != 0xFF
            assert m.sum() >= G // 4
            assert np.array_equal(o_h.cpu().numpy().view(po.HDR_DTYPE).reshape(G, E)[m], x_h[m])
            assert np.array_equal(o_s[:, :, :16].cpu().numpy()[m], x_s[m])
            assert bool((o_s[:, :, 16:4096] == 0x3C).all()) and bool((o_s[:, :, stride - 4096:] == 0x3C).all())
            assert np.array_equal(sh[:, :, :16].cpu().numpy(), rx) and np.array_equal(
                d_h.cpu().numpy().view(po.HDR_DTYPE).reshape(G, k), rh)
    finally:
        del sh, par
        if E:
            del o_s
        torch.cuda.empty_cache()
