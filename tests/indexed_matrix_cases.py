"""Cases and the engine for rfec_recover_indexed_matrix_out (the one-launch
indexed decode of the sender's full row + column plans of k = 6..16), shared by
the CPU and the GPU tests of test_recover_indexed_matrix.py.

Everything else is indexed_cases.py's: a case is its (plan, geometry, groups,
per_group, sparse) tuple, make_inputs builds the pool, the map and the tables,
reference / compare / conditions / swap_two_members judge the outputs, and the
engines run one call behind a guarded arena.  GpuIndexedMatrix is GpuIndexed
with the new entry in _run: the arena's workspace buffer is not passed.
"""
from __future__ import annotations

import numpy as np

import indexed_cases as ic
import pattern_cases as pc

# tag of rfec_indexed_last_path for this entry (rfec_internal.h): MATRIX | k << 8
MATRIX = 3

# the new plans go where indexed_cases.make_inputs looks plans up (names no other case file uses)
PLANS = ic.PLANS
PLANS["full2x3k6"] = lambda o: pc.full_plan(o, 6)     # k = 6 in rows of 3: the smallest shape
PLANS["full4x4k16"] = lambda o: pc.full_plan(o, 16)   # k = 16 in rows of 4: the largest, 8 lines

# (plan, geometry, groups, per_group, sparse): c1200 has CD = 75, so a wave straddles out slots and groups; c20 a
# tail (stride 48, CD = 2); c15 at 1, 63, 64, 65 and 129 groups the edges of the checker blocks (64 groups each) and
# of the payload blocks; c0 at 600 groups more checker than payload blocks; the sparse pool row indices above 65,535
CASES = [
    ("full3x4k10", "c1200", 4, 10, False), ("full3x4k10", "c1000", 12, 3, False), ("full3x4k10", "c20", 7, 3, False),
    ("full3x4k10", "c15", 1, 2, False), ("full3x4k10", "c15", 63, 2, False), ("full3x4k10", "c15", 64, 2, False),
    ("full3x4k10", "c15", 65, 2, False), ("full3x4k10", "c15", 129, 2, False), ("full3x4k10", "c0", 600, 3, False),
    ("full3x4k10", "c0", 7, 3, True),
    ("full2x3k6", "c15", 65, 6, False), ("full4x4k16", "c20", 7, 5, False),
]

# plans the entry refuses (each a valid plan of rfec_recover_indexed_out)
REFUSED = {
    "rows10x4": lambda o: ic.PLANS["rows10x4"](o),
    "hand6": lambda o: ic.PLANS["hand6"](o),                      # k = 6, but not the full matrix
    "strip65": lambda o: ic.PLANS["strip65"](o),
    "k10col3": lambda o: o.plan_matrix(10, 4, 3, ic.rc.ROWS | ic.rc.COLS),  # a full matrix of k = 10 in rows of 3
    "k5": lambda o: o.plan_matrix(5, 2, 3, ic.rc.ROWS | ic.rc.COLS),
    "k17": lambda o: o.plan_matrix(17, 5, 4, ic.rc.ROWS | ic.rc.COLS),
}


def conditions(x, ref):
    """indexed_cases.conditions, with the refused line read as a full matrix shows it.  make_inputs zeroes the
    data_size of group 1's first row parity and loses member 0 alone, so the header checks refuse row 0
    (flex_fec_xor.c:88-89: a present member is longer than fec_data_size).  indexed_cases' reading also wants the
    target left unrecovered, which holds for a row layout and never for these plans: column 0 fires for member 0.
    Here: the row's parity arrived, member 0 is its only missing member, a present member of the row is longer than
    its fec_data_size -- and the reference recovered member 0 all the same, with the sender's header record, which
    only the column can give (the row's meta XOR differs: its data_size was zeroed)."""
    c = ic.conditions(x, ref)
    e_sh, e_hd, e_ix, e_rec = ref
    c["refused_line"] = False
    if x.refused_line is not None:
        g, l = x.refused_line
        k = x.k
        pres = ic.ga.present_rows(x.present, k).reshape(x.G, k)
        mem = x.plan.members(l)
        miss = [i for i in mem if not pres[g, i]]
        c["refused_line"] = bool(
            (int(x.parity_present[g]) >> l) & 1 and miss == [0] and int(e_ix[g, 0]) == 0 and int(e_rec[g, 0]) & 1 and
            any(pres[g, i] and x.hdr["size"][g, i] > x.fec_size[g, l] for i in mem) and
            e_hd[g, 0].tobytes() == x.batch.hdr[g, 0].tobytes())
    return c


class GpuIndexedMatrix(ic.GpuIndexed):
    """One rfec_recover_indexed_matrix_out call behind indexed_cases' arena; rows is NULL for an empty pool."""

    def _workspace_size(self, x):
        return 16  # none is passed: the arena's workspace buffer only has to stay as it was

    def _run(self, x, A):
        self.lib.recover_indexed_matrix_out(x.plan, x.G, x.stride, x.capacity, A.ptr("rows") if x.n_rows else None,
                                            x.n_rows, A.ptr("src_of"), A.ptr("hdr"), A.ptr("present"), A.ptr("meta"),
                                            A.ptr("fec_size"), A.ptr("parity_present"), A.ptr("recovered"), x.E,
                                            A.ptr("out_shards"), A.ptr("out_hdr"), A.ptr("out_index"),
                                            self.torch.cuda.current_stream(self.device).cuda_stream)
        self.last_path = int(self.lib.lib.rfec_indexed_last_path())


def empty_pool_inputs(oracle, G=5, E=3, geom="c20"):
    """All-absent tables over an empty pool: no member, no parity, every map word NONE."""
    capacity, stride = ic.GEOMS[geom]
    plan = ic.PLANS["full3x4k10"](oracle)
    k, n = plan.k, plan.n_lines
    x = ic.Inputs()
    x.case = ("full3x4k10", geom, G, E, False)
    x.plan, x.G, x.k, x.nl, x.E = plan, G, k, n, E
    x.capacity, x.stride = capacity, stride
    x.rows, x.n_rows = np.zeros((0, stride), np.uint8), 0
    x.src_of = np.full(G * (k + n), ic.NONE, np.uint32)
    x.hdr = np.zeros((G, k), ic.po.HDR_DTYPE)
    x.hdr.view(np.uint8)[...] = 0xA5
    x.meta = np.zeros((G, n), ic.po.HDR_DTYPE)
    x.meta.view(np.uint8)[...] = 0xA5
    x.fec_size = np.full((G, n), 7, np.uint16)
    x.present = np.zeros((G, 2), np.uint64)
    x.parity_present = np.zeros(G, np.uint64)
    return x
