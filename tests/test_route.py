"""The PS_MMSE route planner (csrc/wce_route.cpp, through wce_debug_route) against
the kernels wce_estimate actually launched: tests/golden/mmse_routes.json holds,
for every combination of the facts the dispatch consults, the kernel names a
rocprofv3 kernel trace recorded on an MI355X (tests/golden/make_mmse_routes.py;
the file's provenance names the commit the trace came from -- the one before
the planner existed, so the table is the old dispatch's, not the planner's).

No GPU here: the planner is host code.  A family name stands for one launcher;
FAMILIES lists the kernels that launcher may start (the choice among them
depends on the batch size or the device and stays inside the launcher).
"""
import itertools
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))

# family -> the launches it makes, each a set of kernel names it may be; a name
# without template arguments admits every instantiation
FAMILIES = {
    "ls": [{"ls_kernel", "ls_elem_kernel"}],
    "ref_fc": [{"ref_fc_kernel<false>"}],
    "fc_u": [{"ref_fc_kernel<true>"}],
    "matvec": [{"matvec_kernel<false, false, 1>"}],
    "ref_w": [{"ref_w_kernel"}],
    "cm": [{"cm_real_kernel"}, {"cm_cplx_kernel"}],
    "ref_pilots": [{"mmse_ref_flat_kernel", "mmse_ref_elem_kernel"}],
    "ref_ls_elem": [{"ref_ls_elem_kernel"}],
    "ref_ls_elem_done": [{"ref_ls_elem_kernel"}],
    "mmse_rank1": [{"mmse_rank1_kernel<false>"}],
    "mmse_rank1_nt": [{"mmse_rank1_kernel<true>"}],
    "factor_bordered": [{"mmse_solve_fc_kernel"}],
    "factor_rank1_build": [{"mmse_solve_kernel<true>"}],
    "factor_dense": [{"mmse_solve_kernel<false>"}],
    "fused_bordered": [{"mmse_solve_ls_kernel<true, true, true>", "mmse_solve_ls_kernel<true, true, false>"}],
    "fused_rank1_build": [{"mmse_solve_ls_kernel<true, false, true>", "mmse_solve_ls_kernel<true, false, false>"}],
    "fused_dense": [{"mmse_solve_ls_kernel<false, false, true>", "mmse_solve_ls_kernel<false, false, false>"}],
    "mmse_lr": [{"mmse_lr_kernel", "mmse_lr_lane_kernel", "mmse_lr_lane_staged_kernel", "mmse_lr_quad_kernel",
                 "mmse_lr_quad2_kernel"}],
    "fc_finish": [{"fc_finish_kernel"}],
    "matvec_avg": [{"matvec_kernel<false, false, 4>"}],
    "apply": [{"apply_kernel"}],
    "avg_blocks": [{"avg_blocks_kernel"}],
}
EINVAL = -1


@pytest.fixture(scope="module")
def table():
    with open(os.path.join(HERE, "golden", "mmse_routes.json")) as f:
        doc = json.load(f)
    assert doc["columns"] == ["mode", "bdot", "fuse", "cm", "lr_k0", "rank", "sem", "mask", "f32", "r1", "ref_fc", "ref_ls",
                              "rc", "route"]
    assert len(doc["provenance"]["commit"]) == 40
    return doc


def _admits(allowed, kernel):
    return kernel in allowed or kernel.split("<")[0] in allowed


def _matches(families, kernels):
    want = [k for f in families for k in FAMILIES[f]]
    return len(want) == len(kernels) and all(_admits(a, k) for a, k in zip(want, kernels))


def test_planner_matches_recorded_launches(wce, table):
    routes = [r.split(";") if r else [] for r in table["routes"]]
    assert len(table["rows"]) > 1000
    used, bad = set(), []
    for *facts, rc, ri in table["rows"]:
        assert rc == 0, facts   # the walk made only calls the API accepts
        fams = [f for f in wce.debug_route(*facts).split(";") if f]
        used.update(fams)
        if not _matches(fams, routes[ri]):
            bad.append((facts, fams, routes[ri]))
    assert not bad, f"{len(bad)} rows differ, first: {bad[0]}"
    assert used == set(FAMILIES), sorted(set(FAMILIES) - used)   # the walk reached every family


def test_planner_is_deterministic(wce, table):
    """The same facts give the same route, whatever was planned in between."""
    rows = table["rows"][::7]
    first = [wce.debug_route(*r[:12]) for r in rows]
    again = [wce.debug_route(*r[:12]) for r in reversed(rows)]
    assert first == again[::-1]


def test_rejected_facts_are_not_in_the_table(wce, table):
    """What wce_estimate's validation rejects before planning has no route: wce_debug_route says
    so, and the walk recorded none."""
    FC, PS = wce.FRAME_COV, wce.PS_MMSE
    bad = []
    for mode, sem, mask in itertools.product((0, 1, 2, 3, -1), (0, 1, 2), (PS, FC, FC | wce.LT_LS, 0x80 | PS, 0x100)):
        if mode in (0, 1, 2) and sem in (0, 1) and mask == PS:
            continue
        bad.append((mode, 1, 1, 0, -1, 0, sem, mask, 0, 0, 0, 0))
    bad.append((wce.MMSE_REF, 1, 1, 0, 3, 4, 0, PS, 0, 0, 0, 0))        # a low-rank row off a COV context
    bad.append((wce.MMSE_TEXTBOOK, 1, 1, 1, -1, 0, 0, PS, 0, 0, 0, 0))   # a modulus off a COV context
    for facts in bad:
        with pytest.raises(wce.WceError) as e:
            wce.debug_route(*facts)
        assert e.value.code == EINVAL, facts
    for *facts, rc, ri in table["rows"]:
        mode, _, _, cm, k0, _, sem, mask = facts[:8]
        assert mode in (0, 1, 2) and sem in (0, 1) and not mask & ~0x7F and (not mask & FC or mask & PS), facts
        assert mode == wce.MMSE_COV or (k0 < 0 and not cm), facts


def test_short_buffer_is_an_error(wce):
    import ctypes
    buf = ctypes.create_string_buffer(4)
    args = (wce.MMSE_TEXTBOOK, 1, 1, 0, -1, 0, wce.SEM_MATLAB, wce.ALL | wce.FRAME_COV, 0, 0, 0, 0)
    assert wce.load().wce_debug_route(*args, buf, len(buf)) == EINVAL
    assert wce.debug_route(*args) == "ls;matvec;mmse_rank1;fc_finish"
