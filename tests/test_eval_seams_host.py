"""No GPU: the seam table of the evaluation kernels (tests/eval_seams.py).  The constants it reads from the .hip sources are the
ones its shapes were chosen for, and mc_rollout_blocks exports the same block count; every path class the kernel-level tests had
never taken is taken by a table entry, every entry takes the class it is listed for, and no earlier size did; an f64 numpy
evaluation in the kernels' own summation order meets every gate on every new shape, so the gates need no widening; and the
comparisons the GPU tests use reject a mutant confined to each new path, at the shape that path is listed for, while the
earlier sizes pass it."""
import ast
import os
import re

import numpy as np
import pytest

import ensemble_stats_ref as E
import eval_seams as S
import fields
import rollout_score_ref as R
import series_score_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
NEW_ROLLOUT = S.MEMBER_SHAPES + S.WIDTH_SHAPES + S.CHUNK_SHAPES
NEW_SERIES = S.SERIES_SHAPES + [S.GATHER_SHAPE]


# ---- the constants ----------------------------------------------------------------------------------------------------------------
def test_constants_are_the_ones_the_table_was_chosen_for():
    assert S.C == S.EXPECTED, {k: (S.C[k], S.EXPECTED[k]) for k in S.C if S.C[k] != S.EXPECTED.get(k)}
    assert S.FIN_WAVES == 4 and S.C["FIN_LANE_STRIDE"] == S.C["WALK_LANES"] == S.C["WALK_TAIL"] == S.C["SS_LANES"] == 64
    assert S.C["WALK_AHEAD"] == (S.C["WALK_QUADS"] - 1) * S.C["WALK_LANES"] and S.C["WALK_MAIN"] == S.C["WALK_QUADS"] * S.C["WALK_LANES"]
    assert S.C["SS_CHUNK"] <= S.C["SS_LANES"]                  # k_series_finalize stages a chunk with one lane a row
    assert S.C["MEMBER_DIV"] == S.C["MEMBER_BLOCK"] and S.C["GATHER_THREADS"] == S.C["GATHER_BLOCK"]


def test_rollout_blocks_is_what_the_library_exports():
    from pbml_mantle_convection_amd import _lib as L
    lib = L.load()
    for h, w in [(5, 5), (5, 6), (9, 70), (16, 16), (16, 17), (33, 130), (128, 255), (128, 256), (128, 257), (130, 260), (128, 506),
                 (506, 506), (513, 520)] + [(H, W) for _, H, W in NEW_ROLLOUT]:
        assert lib.mc_rollout_blocks(h, w) == S.rollout_blocks(h, w), (h, w)
    assert S.rollout_blocks(5, 5) == 1 and S.rollout_blocks(128, 256) == 128 == S.rollout_blocks(506, 506)


def test_the_earlier_sizes_are_the_ones_the_test_files_hold():
    def sizes(name):
        src = open(os.path.join(HERE, name)).read()
        return ast.literal_eval(re.search(r"^SIZES = (\[.*?\])", src, re.M).group(1))
    assert sizes("test_hip_rollout.py") == S.OLD_ROLLOUT and sizes("test_hip_series_score.py") == S.OLD_SERIES
    net = open(os.path.join(HERE, "test_hip_rollout_net.py")).read()
    assert re.search(r"^B, H, W = 3, 32, 48$", net, re.M) and (3, 32, 48) in S.OLD_NET_ROLLOUT
    net = open(os.path.join(HERE, "test_hip_series_score_net.py")).read()
    assert re.search(r"^N, H, W, BATCH = 5, 64, 90, 2$", net, re.M) and S.OLD_NET_SERIES == [(5, 64, 90)]


# ---- coverage ---------------------------------------------------------------------------------------------------------------------
def test_every_entry_takes_the_path_it_is_listed_for():
    assert sorted(S.ROLLOUT_PATHS) == sorted(NEW_ROLLOUT) and sorted(S.SERIES_PATHS) == sorted(NEW_SERIES)
    for shape, want in list(S.ROLLOUT_PATHS.items()) + list(S.SERIES_PATHS.items()):
        got = S.paths(shape)
        for k, v in want.items():
            assert got[k] == v, (shape, k, got[k], v)
    # per lane: 0-57 and 58-63 part ways
    assert [S.walk_lane(250, l) for l in (0, 57, 58, 63)] == [(1, 0), (1, 0), (0, 3), (0, 3)]
    assert [S.walk_lane(506, l) for l in (0, 57, 58, 63)] == [(2, 0), (2, 0), (1, 3), (1, 3)]
    assert S.walk_columns(506, 58) == [58, 122, 186, 250, 314, 378, 442] and S.walk_columns(506, 57)[-1] == 505
    for W in (5, 6, 70, 130, 250, 260, 506):                   # every column once, ascending within a lane
        cols = [S.walk_columns(W, l) for l in range(64)]
        assert sorted(sum(cols, [])) == list(range(W)) and all(c == sorted(c) for c in cols)


def test_every_new_path_class_is_taken_and_no_earlier_size_took_it():
    old_r, old_s = S.OLD_ROLLOUT + S.OLD_NET_ROLLOUT, S.OLD_SERIES + S.OLD_NET_SERIES
    classes = {
        # k_series_finalize: a second pass; a last pass shorter than a chunk after a full one; a third pass; exactly one full pass
        "finalize two passes": (NEW_SERIES, old_s, lambda p: p["series_finalize"][0] >= 2),
        "finalize short last pass": (NEW_SERIES, old_s, lambda p: p["series_finalize"][0] >= 2 and p["series_finalize"][1] < S.C["SS_CHUNK"]),
        "finalize three passes": (NEW_SERIES, old_s, lambda p: p["series_finalize"][0] >= 3),
        # k_rollout_finalize: a second member iteration; a trip count that differs between the waves
        "finalize second member": (NEW_ROLLOUT, old_r, lambda p: max(p["finalize_members"]) >= 2),
        "finalize ragged waves": (NEW_ROLLOUT, old_r, lambda p: max(p["finalize_members"]) >= 2 and len(set(p["finalize_members"])) > 1),
        # the per-member kernels: block 1
        "member block 1": (NEW_ROLLOUT, old_r, lambda p: p["member_blocks"][0] >= 2),
        # rs_walk_row: lanes split between the loops; two main passes; the deployed width's mix
        "walk split wave": (NEW_ROLLOUT, old_r, lambda p: {m for m, _ in p["walk_row"]} == {0, 1}),
        "walk two main passes": (NEW_ROLLOUT, old_r, lambda p: max(m for m, _ in p["walk_row"]) >= 2),
        "walk deployed mix": (NEW_ROLLOUT, old_r, lambda p: p["walk_row"] == S.walk_row(506) == {(2, 0), (1, 3)}),
        # rs_score_row: exactly one chunk; a one-row second chunk with fifteen idle waves
        "score one full chunk": (NEW_ROLLOUT, old_r, lambda p: p["score_chunks"] == (1, S.C["RS_CHUNK"], 0)),
        "score one-row chunk": (NEW_ROLLOUT, old_r, lambda p: p["score_chunks"] == (2, 1, S.C["RS_WAVES"] - 1)),
        # k_series_build_input: the grid-stride pass
        "gather second pass": (NEW_SERIES, old_s, lambda p: p["gather_passes"] >= 2),
    }
    for name, (new, old, takes) in classes.items():
        assert any(takes(S.paths(s)) for s in new), name
        assert not any(takes(S.paths(s)) for s in old), (name, [s for s in old if takes(S.paths(s))])
    assert S.paths((5, 64, 90))["series_finalize"] == (1, 64)  # (the network test: exactly one pass; kernel level had none)
    # the deployed grids take what the table takes
    assert S.series_finalize(128) == (2, 64) and S.series_finalize(506) == (8, 58) and S.score_chunks(506) == (4, 122, 0)
    assert S.walk_row(506) == S.paths((2, 5, 506))["walk_row"] and S.gather_passes(506, 506) == 1 and S.gather_passes(513, 520) == 2


# ---- the host cases ---------------------------------------------------------------------------------------------------------------
def score_fields(B, H, W, m):
    """Member m's state before the step, a state after it and a truth snapshot, f32 (the GPU test's T, a smooth change of about
    0.01, its truth fields)."""
    Tp = S.rollout_fields(B, H, W)[2][m].astype(np.float32)
    Tn = (Tp + 0.1 * fields.smooth_field(B, H, W, 7000 + H)[m]).astype(np.float32)
    Tr = fields.temperature_field(B * 2, H, W, 9000 + H).astype(np.float32)[2 * m]
    return Tp, Tn, Tr


def series_item(N, H, W, j):
    f = S.series_fields(N, H, W)
    inv = S.INV[f["sim"][j]]
    sc = lambda a: Q.scaled(a.astype(np.float32), inv)  # noqa: E731
    p = int(f["prev"][j])
    ub, vb = (sc(f["u"][p]), sc(f["v"][p])) if p >= 0 else (None, None)
    return S.series_rows(f["pred"][j, 0].astype(np.float64), f["pred"][j, 1].astype(np.float64), sc(f["u"][j]), sc(f["v"][j]), ub, vb)


def series_reference(N, H, W):
    f = S.series_fields(N, H, W)
    return Q.score(f["pred"][:, 0], f["pred"][:, 1], f["u"].astype(np.float32), f["v"].astype(np.float32), f["sim"], f["prev"], S.INV,
                   list(range(N)))


def series_passes(N, H, W, mutant=None):
    """test_table_and_profile_against_numpy's comparison on the kernel-order evaluation (of a mutant)."""
    table, profile, gate, pgate = series_reference(N, H, W)
    got = [S.series_finalize_ordered(series_item(N, H, W, j), W, mutant) for j in range(N)]
    t, p = np.stack([g[0] for g in got]), np.stack([g[1] for g in got])
    worst = max(S.worst_ratio(t, table, gate), S.worst_ratio(p, profile, pgate))
    return bool(np.array_equal(t[:, Q.MAX_COLS], table[:, Q.MAX_COLS])) and Q.close(t, table, gate) and Q.close(p, profile, pgate), worst


def score_passes(B, H, W, mutant=None, m=0, theta=0.3):
    Tp, Tn, Tr = score_fields(B, H, W, m)
    ref = R.score_row(Tp, Tn, Tr, 1.25, theta)
    row, prof = S.score_row_ordered(Tp, Tn, Tr, 1.25, theta, mutant)
    worst = max(S.worst_ratio(row, ref["row"], ref["gate"]), S.worst_ratio(prof, ref["prof"], ref["gate_prof"]))
    return S.score_row_passes(row, prof, ref), worst


# ---- the kernels' order meets the gates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", NEW_ROLLOUT)
def test_kernel_order_meets_the_rollout_score_and_profile_gates(B, H, W):
    for m in sorted({0, B - 2, min(B - 1, 5)}):
        for theta in (0.3, 1.0):
            ok, worst = score_passes(B, H, W, None, m, theta)
            print(f"{B} x {H} x {W} member {m} theta {theta}: rollout score in kernel order, worst err / gate {worst:.3e}")
            assert ok and worst <= 1.0
    u, v, T = S.rollout_fields(B, H, W)
    vs = S.member_scalars(B)[0]
    want, mag = E.profiles(u, v, vs, T)
    got = S.profiles_ordered(u, v, vs, T)
    worst = S.worst_ratio(got, want, 1e-12 * mag / W)
    print(f"{B} x {H} x {W}: profiles in kernel order, worst err / gate {worst:.3e}")
    assert (np.abs(got - want) <= 1e-12 * mag / W).all()


@pytest.mark.parametrize("N,H,W", S.SERIES_SHAPES)
def test_kernel_order_meets_the_series_gates(N, H, W):
    ok, worst = series_passes(N, H, W)
    print(f"{N} x {H} x {W}: series table and profile in kernel order, worst err / gate {worst:.3e}")
    assert ok and worst <= 1.0


def test_the_added_additions_stay_inside_the_fixed_gate():
    """1e-12 is the project's figure; the longest chain a new shape adds is H = 130 rows after 6 tree levels and one column:
    137 additions, 137 * 2^-53 = 1.5e-14 of sum|terms|."""
    assert (130 + 6 + 1) * 2.0 ** -53 < 1.6e-14 < 1e-12 and R.depth(129, 5) == 1 + 6 + 129 + 8 and R.depth(5, 506) == 8 + 6 + 5 + 8


# ---- mutants: the series table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", S.SERIES_MUTANTS)
def test_series_mutants(mutant):
    # a second pass of one row: seen, but for the maxima, none of which lies in row 64 of these fields (the comparison is exact,
    # so it is the fields that decide; at 130 rows they do, see below)
    assert series_passes(2, 65, 5, mutant)[0] == (mutant == "first_pass_maxima")
    assert not series_passes(3, 130, 9, mutant)[0]             # 64 + 64 + 2 rows: every mutant is seen
    assert series_passes(2, 64, 5, mutant)[0]                  # exactly one pass: nothing to lose
    for N, H, W in S.OLD_SERIES + S.OLD_NET_SERIES:            # the old table could not see any of them
        assert series_passes(N, H, W, mutant)[0], (N, H, W)


def test_a_maximum_lies_beyond_the_first_pass():
    """first_pass_maxima is seen because at 3 x 130 x 9 a table maximum lies in a row >= 64 (exact comparison)."""
    rows = np.stack([series_item(3, 130, 9, j) for j in range(3)])
    assert (rows[:, 4:8, 64:].max(-1) > rows[:, 4:8, :64].max(-1)).any()


# ---- mutants: a rollout-score row ------------------------------------------------------------------------------------------------------
def test_width_mutants():
    assert not score_passes(2, 5, 506, "drop_tail_after_main_lanes_58")[0]
    assert not score_passes(2, 5, 250, "drop_tail_only_lanes")[0]
    assert score_passes(2, 5, 250, "drop_tail_after_main_lanes_58")[0] and score_passes(2, 5, 506, "drop_tail_only_lanes")[0]       # each its own width
    for B, H, W in S.OLD_ROLLOUT:
        for mutant in ("drop_tail_after_main_lanes_58", "drop_tail_only_lanes"):
            assert score_passes(B, H, W, mutant)[0], (B, H, W, mutant)


@pytest.mark.parametrize("mutant", ["reset_at_one_row_chunk", "bars_without_one_row_chunk"])
def test_chunk_mutants_confined_to_the_one_row_chunk(mutant):
    assert not score_passes(2, 129, 5, mutant)[0]
    assert score_passes(2, 128, 5, mutant)[0]
    for B, H, W in S.OLD_ROLLOUT:                              # 130 x 260 included: its second chunk holds two rows
        assert score_passes(B, H, W, mutant)[0], (B, H, W)


@pytest.mark.parametrize("mutant", ["reset_at_chunk", "bars_first_chunk"])
def test_chunk_mutants_at_every_boundary(mutant):
    """The same two errors at EVERY chunk boundary: seen at 129 rows, and also by the one earlier size with a second chunk
    (130 x 260) -- what that size could not see is the error that needs a chunk of one row (above)."""
    assert not score_passes(2, 129, 5, mutant)[0] and score_passes(2, 128, 5, mutant)[0]
    for B, H, W in S.OLD_ROLLOUT:
        assert score_passes(B, H, W, mutant)[0] == (H <= S.C["RS_CHUNK"]), (B, H, W)


# ---- mutants: the per-member kernels ---------------------------------------------------------------------------------------------------
def member_checks(got, ref, B, H, W):
    """What test_hip_rollout asserts of a free step, on numpy arrays: dt finite, positive and the member's own; flags, clocks and
    counts; every member's diagnostics against its own fields."""
    try:
        assert np.isfinite(got["dt"]).all() and (got["dt"] > 0).all() and got["dt"].tolist() == ref["dt"].tolist()
        assert got["flags"].tolist() == [1] * B and got["t"].tolist() == got["dt"].tolist() and got["steps"].tolist() == [1] * B
        assert got["hist"][:, 1].tolist() == got["dt"].tolist() and got["hist"][:, 0].tolist() == got["dt"].tolist()
        for b in range(B):
            Tn = ref["T"][b].astype(np.float32).astype(np.float64)
            S.diagnostics_check(got["hist"][b], Tn, ref["u"][b].astype(np.float64), ref["v"][b].astype(np.float64), np.float64(ref["vs"][b]),
                                ref["yc"], b)
    except AssertionError:
        return False
    return True


@pytest.mark.parametrize("B,H,W", S.MEMBER_SHAPES)
def test_member_cases_are_what_the_gpu_tests_assume(B, H, W):
    r = S.rollout_host(B, H, W)
    assert len(set(r["dt"].tolist())) == B and (r["dt"][:B - 1] < r["diffusive"]).all() and r["dt"][B - 1] == r["diffusive"]
    vs, raq = S.member_scalars(B)
    assert len(set(vs.astype(np.float32).tolist())) == B and len(set(raq.astype(np.float32).tolist())) == B
    assert len({round(float(x), 12) for x in r["hist"][:, 2]}) == B                        # different fields
    assert member_checks(r, r, B, H, W)
    for last in (S.FROZEN, S.STEP, S.LAND):
        role = S.roles(B, last)
        assert role[:2] == [S.FROZEN, S.LAND] and role[4:6] == [S.FROZEN, S.LAND] and {S.FROZEN, S.STEP, S.LAND} == set(role[:4]) | {S.STEP}
        if B > 256:
            assert role[253:256] == [S.LAND, S.STEP, S.FROZEN] and role[256] == last
    assert S.named_members(B) == [m for m in (4, 5, 255, 256) if m < B] and S.named_members(4) == []
    # the stopping rule on the host model: who freezes, who lands, and the clocks they are left with
    role = S.roles(B, S.LAND)
    t_end = [0.5 if role[b] == S.FROZEN else (1.0 + 0.3 * r["dt"][b] if role[b] == S.LAND else np.inf) for b in range(B)]
    g = S.rollout_host(B, H, W, t0=[1.0] * B, t_end=t_end, steps0=[5 + b for b in range(B)])
    assert g["flags"].tolist() == role
    for b in range(B):
        want_t = (1.0, 1.0 + r["dt"][b], t_end[b])[role[b]]
        assert g["t"][b] == want_t and g["steps"][b] == 5 + b + (role[b] != S.FROZEN), b


@pytest.mark.parametrize("mutant", S.MEMBER_MUTANTS)
def test_member_mutants(mutant):
    for B, H, W in S.MEMBER_SHAPES:
        ref, got = S.rollout_host(B, H, W), S.rollout_host(B, H, W, mutant=mutant)
        seen = not member_checks(got, ref, B, H, W)
        assert seen == (mutant != "unset_from_256" or B > 256), (B, mutant)
    for B, H, W in [(3, 5, 6), (2, 9, 70), (4, 33, 130)]:      # at most four members, one block: nothing to see
        ref, got = S.rollout_host(B, H, W), S.rollout_host(B, H, W, mutant=mutant)
        assert member_checks(got, ref, B, H, W), (B, mutant)


def test_stopping_mutants_are_seen_by_the_stopping_assertions():
    """clocks_stop_at_4 under the stopping test's clocks: the landing member 5 keeps t = 1 where t_end is asserted."""
    B, H, W = 6, 9, 70
    free = S.rollout_host(B, H, W)
    role = S.roles(B, S.LAND)
    t_end = [0.5 if role[b] == S.FROZEN else (1.0 + 0.3 * free["dt"][b] if role[b] == S.LAND else np.inf) for b in range(B)]
    got = S.rollout_host(B, H, W, t0=[1.0] * B, t_end=t_end, steps0=[5 + b for b in range(B)], mutant="clocks_stop_at_4")
    assert got["t"][1] == t_end[1] and got["steps"][1] == 7    # below four: as asserted
    assert got["t"][5] == 1.0 != t_end[5] and got["steps"][5] == 10 != 11
