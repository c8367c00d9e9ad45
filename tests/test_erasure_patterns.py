"""The exhaustive erasure-pattern sweep (pattern_cases.py) of the decoders of the
sender's matrix plans, k = 6..16.  On the CPU: the vectorised mask model against
packed_matrix_cases.mask_schedule and against the oracle on every pattern, the
censuses that keep the sweep honest, the oracle behind the guarded arena through
every check, and the self-test that the checks can fail.  On the GPU: every
decoder of these plans on every pattern, clean and tampered, each asserting the
dispatch tag of the kernel it is written for."""
import time

import numpy as np
import pytest

import geometry_cases as gc
import guarded_arena as ga
import pattern_cases as pc

SWEEPS = [(k, "s16") for k in pc.KS] + [(k, "s48") for k in pc.S48_KS]
SWEEP_IDS = [f"k{k}-{g}" for k, g in SWEEPS]


# -- CPU -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", pc.KS)
def test_model_is_mask_schedule(oracle1000, k):
    """The plan is the sender's (5, 5, 6, 6, 7, 7, 7, 7, 8, 8, 8 lines for k = 6..16, rows of 3 up to k = 9, then of
    4), the sweep has the groups the issue sets, and the vectorised model equals mask_schedule on a seeded sample at
    every per_group."""
    plan = pc.full_plan(oracle1000, k)
    mm, ppm = pc.pattern_masks(k, plan.n_lines)
    assert len(mm) == (1 << (k + plan.n_lines) if k <= 10 else 3 << k)
    if k > 10:  # every count of lost parities occurs
        assert set(pc.popcount(ppm).tolist()) == set(range(plan.n_lines + 1))
    for E in pc.PER_GROUP(k):
        pc.check_model_sample(plan, mm, ppm, E)


def test_sweep_sizes():
    assert [pc.N_LINES[k] for k in range(6, 11)] == [5, 5, 6, 6, 7]
    assert [pc.N_LINES[k] for k in range(10, 17)] == [7, 7, 7, 7, 8, 8, 8]
    assert len(pc.pattern_masks(10, 7)[0]) == 131072 and len(pc.pattern_masks(16, 8)[0]) == 196608


@pytest.mark.parametrize("k,geom", SWEEPS, ids=SWEEP_IDS)
def test_clean_sweep_oracle(oracle1000, k, geom):
    """Nothing tampered: on every pattern the oracle (behind the guarded arena) recovers exactly the model's mask,
    in place and at every per_group, and every recovered header and slot equals the original group's.  The
    schedule-length census holds: every length up to the largest occurs, the largest is >= 5 from k = 7, 7 for
    k = 13..16 and never above the 8 steps a schedule record holds."""
    sw = pc.sweep(oracle1000, k, geom, "clean")
    print(f"{sw.name()}: {sw.G} groups, schedule lengths {pc.clean_census(sw)}")
    eng = ga.OracleArenaEngine(oracle1000)
    pc.run_in_place(eng, sw)
    for E in pc.PER_GROUP(k):
        pc.run_dense(eng.recover_out, sw, E)


@pytest.mark.parametrize("k,geom", SWEEPS, ids=SWEEP_IDS)
def test_tampered_sweep_oracle(oracle1000, k, geom):
    """One header corruption per group: the oracle's recovered set is a subset of the model's, in place and at
    every per_group; the census of rejected groups (>= 1 % rejected, >= 1 % rejected with a cascade, from k = 8
    >= 0.5 % rejected with more than 4 steps) holds on the oracle's own result; and the oracle behind the guarded
    arena passes every check."""
    sw = pc.sweep(oracle1000, k, geom, "tampered")
    print(f"{sw.name()}: {pc.tampered_census(sw)}")
    for E in pc.PER_GROUP(k):
        rec = sw.expected_dense(E)[3][:, 0].astype(np.int64)
        assert not (rec & ~pc.model(sw.plan, sw.mm, sw.ppm, E)[0]).any(), E
    eng = ga.OracleArenaEngine(oracle1000)
    pc.run_in_place(eng, sw)
    for E in pc.PER_GROUP(k):
        pc.run_dense(eng.recover_out, sw, E)


@pytest.mark.parametrize("wrong", pc.WRONG)
def test_checks_catch_wrong_engine(oracle1000, wrong):
    """Each engine that is wrong on purpose is caught, and the report names the groups with their masks and step
    counts."""
    k, variant, E, words = {"drops_long": (10, "clean", 10, ["recovered masks differ"]),
                            "mask_peel": (10, "tampered", 10, ["recovered masks differ"]),
                            "swapped_slots": (10, "clean", 3, ["out slots differ", "1 groups"]),
                            "flipped_byte": (16, "clean", 0, ["recovered slots differ", "1 groups", "7 steps"]),
                            "flipped_header": (10, "tampered", 0, ["recovered header records differ", "1 groups"]),
                            "wrong_index": (10, "tampered", 4, ["out_index differs", "1 groups"])}[wrong]
    sw = pc.sweep(oracle1000, k, "s16", variant)
    eng = pc.WrongEngine(ga.OracleArenaEngine(oracle1000), sw, wrong)
    with pytest.raises(AssertionError) as e:
        if E:
            pc.run_dense(eng.recover_out, sw, E)
        else:
            pc.run_in_place(eng, sw)
    msg = str(e.value)
    assert all(w in msg for w in words + ["members 0x", "parities 0x", "steps)"]), msg
    if wrong in ("drops_long", "mask_peel"):
        with pytest.raises(AssertionError, match="recovered masks differ"):
            pc.run_in_place(eng, sw)
    if wrong == "drops_long":  # every group it reports has a schedule of more than 4 steps
        assert " 5 steps" in msg or " 6 steps" in msg


# -- GPU -----------------------------------------------------------------------------------------------------------------
# decoder -> (tuning, dispatch tag of k)
DECODERS = {
    "in_place": (0, lambda k: gc.tag("CASCADE", 32)),
    "in_place_generic": (gc.TUNE_GENERIC, lambda k: gc.tag("PEEL_FLAT", 4 | gc.FAST)),
    "dense": (0, lambda k: gc.tag("MATRIX_DENSE", k)),
    "dense_plan_cascade": (gc.TUNE_PLAN_CASCADE, lambda k: gc.tag("CASCADE_DENSE", 32)),
    "dense_generic": (gc.TUNE_GENERIC, lambda k: gc.tag("PEEL_FLAT", 4 | gc.FAST | gc.DENSE)),
    "packed": (0, lambda k: gc.tag("MATRIX_PACKED", k)),
    "indexed": (0, None),
}
GPU_CASES = [(k, geom, variant, dec) for k, geom in SWEEPS for variant in pc.VARIANTS for dec in DECODERS]


@pytest.fixture(scope="module")
def gpu_engine():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu suite must run on an MI355X")
    from gpu_engine import GpuEngine
    return lambda tuning: GpuEngine(1000, "cuda:0", tuning, random_workspace=True)


def _tagged(eng, want, what):
    assert eng.last_path == want, f"{what}: took {gc.tag_name(eng.last_path)}, written for {gc.tag_name(want)}"
    return gc.tag_name(want)


@pytest.mark.gpu
@pytest.mark.parametrize("k,geom,variant,decoder", GPU_CASES, ids=["-".join(map(str, c)) for c in GPU_CASES])
def test_erasure_patterns_gpu(gpu_engine, oracle1000, k, geom, variant, decoder):
    """One decoder on every pattern of one sweep: masks, header records and whole slots of every recovered segment
    (dense: out_index too, at per_group 1, 3, 4, 5 and k; the indexed decode at 3 and k) equal the expected ones --
    clean: the model's mask and the original group; tampered: the oracle's."""
    sw = pc.sweep(oracle1000, k, geom, variant)
    t0 = time.time()
    tuning, tag_of = DECODERS[decoder]
    what = f"{sw.name()} {decoder}"
    if decoder == "indexed":
        import indexed_cases as ic
        from razor_amd.fec import native
        for E in (3, k):
            x = pc.indexed_inputs(sw, E)
            eng = ic.GpuIndexed(native(1000))
            got = eng.run(x)
            assert eng.last_path == (ic.PEEL_REPLAY | 4 << 8), f"{what}: path {eng.last_path:#x}"
            pc.check_dense(sw, got, E, what, fill=ic.FILL)
        name = f"PEEL_REPLAY:{4:#x} (rfec_indexed_last_path)"
    elif decoder.startswith("in_place"):
        eng = gpu_engine(tuning)
        pc.check_in_place(sw, eng.recover(*sw.args()), what)
        name = _tagged(eng, tag_of(k), what)
    else:
        eng = gpu_engine(tuning)
        for E in pc.PER_GROUP(k):
            if decoder == "packed":
                got = eng.recover_packed_matrix(*sw.args(), E)[:4]
                assert eng.pack_path == gc.tag("PACK_MATRIX"), gc.tag_name(eng.pack_path)
            else:
                got = eng.recover_out(*sw.args(), E)
            name = _tagged(eng, tag_of(k), f"{what} E={E}")
            pc.check_dense(sw, got, E, what)
    print(f"{what}: {sw.G} groups, dispatch {name}, {time.time() - t0:.2f} s")
