"""K1 / K6 edge cases (tests/k1_cases.py), CPU tier: the golden model against the C++ twin.

Every case runs through ``igaming_platform_amd.golden`` and through ``CpuScorer`` (score, ingest,
state). Result rows and FeatRec rows must agree field by field, and after every step the twin's
whole store - tx rings, HLL registers, AcctRT with the cached estimates, GRU event rows - must
equal :func:`golden_state` byte for byte. That validates the cases, the packer and the host twin
before a GPU sees them (tests/test_k1_edges_gpu.py runs the same cases on the device).

The model-input rows are compared on the device only (rtol 2e-7, the bound of
tests/test_kernels_gpu.py::test_normalized_inputs_match_golden); here the golden ``log_t`` is held
against float64 ``log1p`` at the magnitudes of these cases (sums near 2^45, amounts up to 2^40).
"""
import math

import numpy as np
import pytest

from igaming_platform_amd.golden import hll as GH
from igaming_platform_amd.golden.features import log_t
from igaming_platform_amd.layouts import FEATREC, REQREC, unpack_results

from . import k1_cases as C

CASES = C.all_cases()


def _twin(case, cfg, pop):
    from igaming_platform_amd.engine.backends import NativeCpuBackend
    bl, ip = C.make_tables(case.world)
    cpu = NativeCpuBackend(cfg, case.n_acc, model="heuristic", blacklist=bl, ipintel=ip)
    cpu.set_batch_rows(np.arange(case.n_acc), pop.batch)
    cpu.set_ext(np.arange(case.n_acc), pop.ext)
    return cpu


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_twin_matches_golden(case):
    cfg = case.world.config(case.bucket)
    pop = C.make_pop(case.world, case.batch)
    gold = C.new_golden(case, pop)
    cpu = _twin(case, cfg, pop)
    d = C.state_diff(cpu.sc.state(), C.golden_state(gold, pop, cfg), case.n_acc)
    assert not d, "empty store: " + d
    for q, st in enumerate(case.steps):
        tag = f"{case.name} step {q} ({st.kind})"
        raw = np.ascontiguousarray(st.rows, REQREC).view(np.uint8)
        if st.kind == "ingest":
            cpu.sc.ingest(raw)
            C.apply_rows(gold, pop, st.rows)
        else:
            want = C.golden_rows(cfg, gold, pop, st.rows, st.now)
            res, feat = cpu.sc.score(raw, st.now, st.kind == "score", True)
            C.check_scored(tag, st.rows, want, unpack_results(np.asarray(res)),
                           np.asarray(feat).view(FEATREC).reshape(-1))
            if st.kind == "score":
                C.apply_rows(gold, pop, st.rows, now=st.now)
        d = C.state_diff(cpu.sc.state(), C.golden_state(gold, pop, cfg), case.n_acc)
        assert not d, f"{tag}: {d}"


def test_every_path_meets_every_edge():
    """The path x edge matrix of tests/k1_cases.py is complete: every listed pair has a case whose
    steps select that path (expected_path, from K1_SEG_MAX, DEDUP_LIST and the minimum TTL), no
    case is skipped or expected to fail, and a pair left out on purpose is named with its reason."""
    have = {}
    for c in CASES:
        if c.path:
            assert C.expected_path(c) == c.path, (c.name, C.expected_path(c), C.focus_shape(c))
            have.setdefault((c.path, c.edge), []).append(c.name)
    missing = [(p, e) for e, paths in C.MATRIX.items() for p in paths
               if (p, e) not in have and (p, e) not in C.LEFT_OUT]
    assert not missing, missing
    assert all(reason for reason in C.LEFT_OUT.values()) and all(C.READ_LEFT_OUT.values())
    assert set(have) | set(C.LEFT_OUT) == {(p, e) for e, paths in C.MATRIX.items() for p in paths}
    marks = getattr(test_twin_matches_golden, "pytestmark", [])
    assert [m.name for m in marks] == ["parametrize"] and len(marks[0].args[1]) == len(CASES)
    assert all(isinstance(c, C.Case) for c in marks[0].args[1])   # plain cases: no skip / xfail marks


def test_visits_lie_whole_in_one_step_and_chosen_events_where_named():
    """No visit is split over steps (its multiplicity selects the path), every seg_hot visit has a
    non-empty bulk in front of the hot tail unless the case is about the counts themselves, and
    the chosen HLL events of the hot / scan cases sit where the case's name says: in the hot
    workgroup's bulk (ranks below ctot - T) or in its exact tail (the scan path: the third chunk)."""
    for c in CASES:
        via = "score" if c.path in C.SCORE_PATHS else "ingest"
        for slot, clock in {v[:2] for v in c.visits}:   # (an account may come twice at one clock: two steps)
            got = [int((st.rows["slot"] == slot).sum()) for st in c.steps
                   if st.kind == via and not st.setup and st.now == clock and (st.rows["slot"] == slot).any()]
            assert got == [n for s_, c_, n in c.visits if (s_, c_) == (slot, clock)], (c.name, slot, clock, got)
        T = C.hot_tail(c.world.ev_ring)
        if c.path == "seg_hot" and c.edge in ("ttl", "ring_wrap", "ev_head", "fields", "hll"):
            assert c.visits and all(n - T > 0 for _, _, n in c.visits), (c.name, T)
        if c.edge == "hll" and c.path in ("seg_hot", "ing_scan"):
            assert len(c.chosen) == len(C.HLL_SCENARIOS)
            for slot, first, last, ctot in c.chosen:
                assert (slot, C.NOW, ctot) in c.visits
                nb = ctot - T if c.path == "seg_hot" else 128
                assert (first >= nb) if c.name.startswith("hll_tail") else (last < ctot - T), (c.name, slot, first, last)


def test_rule_cases_meet_the_ml_threshold():
    """ml exactly 0.7 (ml_high_risk_threshold: not above it, no ML_HIGH_RISK) and one ulp past it."""
    case = next(c for c in CASES if c.name == "rules_review50_block80")
    cfg, pop = case.world.config(case.bucket), C.make_pop(case.world, case.batch)
    gold = C.new_golden(case, pop)
    C.apply_rows(gold, pop, case.steps[0].rows)
    at, past, below = C.golden_rows(cfg, gold, pop, case.steps[1].rows, case.steps[1].now)[-3:]
    assert cfg.scoring.ml_high_risk_threshold == 0.7
    assert at["ml"] == 0.7 and "ML_HIGH_RISK" not in at["reasons"]
    assert past["ml"] == np.nextafter(0.7, 1.0) and "ML_HIGH_RISK" in past["reasons"]
    assert below["ml"] < 0.7 and "ML_HIGH_RISK" not in below["reasons"]


def test_case_tables_hold_the_edges_they_name():
    """The constructions the case tables rely on."""
    # the hash makers: chosen register and rank; rank 57 and hash 0
    for reg, rank in ((0, 1), (255, 56), (77, 57), (4, 30)):
        h = C.hash_for(reg, rank, 0xABCDEF)
        assert (h & 255, GH.rank_of(h)) == (reg, rank) and (h != 0 or (reg, rank) == (0, 57))
    assert C.hash_for(0, 57) == 0 and C.hash_for(77, 57) >> 8 == 0
    # one estimate on each side of the switch from linear counting to the harmonic mean, and no zero register
    n = C.hll_switch_n()
    lo, hi = bytearray(GH.M), bytearray(GH.M)
    for j in range(n):
        hi[j] = 30
        if j < n - 1:
            lo[j] = 30
    assert GH.count(lo) == GH.linear_count(GH.M - (n - 1))
    assert GH.count(hi) != GH.linear_count(GH.M - n) and GH.count(hi) == int(GH.ALPHA * GH.M * GH.M / (
        (GH.M - n) + n * 2.0 ** -30) + 0.5)
    # dedup region: the two accounts of the collision cases share a home slot at the store's capacity
    s1, s2 = C.colliding_slots(256)
    assert s1 != s2 and C.mix32(s1) % 512 == C.mix32(s2) % 512 and C.dedup_cap(256) == 512
    # tables: one chain from the last slot over the wrap, found on the last allowed probe
    bl, ip = C.make_tables(C.World(tables="edges"))
    t = bl.table
    assert t.cap == 16 and t.max_probe == 4 and [int(t.keys[i]) for i in (15, 0, 1, 2)] == [C.BL_A, C.BL_B, C.BL_C, C.BL_D]
    assert t.get(C.BL_ABSENT) is None and t.get(C.BL_HIGH_OTHER) is None and t.get(C.BL_HIGH) == 0
    assert ip.table.max_probe == 3 and int(ip.table.keys[1]) == C.IP_C
    # the hot tail of every event ring of the cases, and the ring that outgrows it
    assert [C.hot_tail(e) for e in C.EV_RINGS] == [64, 64, 128, 192, 192] and C.EV_RINGS[-1] > C.HOT_TAIL_MAX
    # hour sums: a carry across bit 32, a sum near 2^45 and below 2^53
    amts = [a for _, a in C.EDGE_ENTRIES]
    assert sum(a for a in amts if a == 0xFFFFFFFF) > 1 << 33 and 1 << 45 < sum(amts) < 1 << 53


def test_rule_cases_reach_the_action_thresholds():
    """The moved review / block thresholds sit on scores the rules case reaches: the same rows are
    reviewed / blocked at the threshold and approved / reviewed one past it."""
    from igaming_platform_amd.config import ACTION_APPROVE, ACTION_BLOCK, ACTION_REVIEW
    acts = {}
    for case in CASES:
        if case.edge != "rules":
            continue
        cfg, pop = case.world.config(case.bucket), C.make_pop(case.world, case.batch)
        gold = C.new_golden(case, pop)
        C.apply_rows(gold, pop, case.steps[0].rows)
        rows = C.golden_rows(cfg, gold, pop, case.steps[1].rows, case.steps[1].now)
        acts[(case.world.review, case.world.block)] = {s: {g["action"] for g in rows if g["score"] == s}
                                                       for s in C.RULE_SCORES}
    lo, hi = C.RULE_SCORES
    assert acts[(lo, hi)] == {lo: {ACTION_REVIEW}, hi: {ACTION_BLOCK}}
    assert acts[(lo + 1, hi + 1)] == {lo: {ACTION_APPROVE}, hi: {ACTION_REVIEW}}
    assert acts[(50, 80)] == {lo: {ACTION_APPROVE}, hi: {ACTION_BLOCK}}


def test_feature_vector_bodies_sit_on_both_sides_of_the_image_limit():
    """The host serializer's length of the FeatureVector boundary rows (k1_cases.fv_case): 125 and
    126 bytes fit a row's 128-byte image, 127 does not; a row without an account has an empty body."""
    from igaming_platform_amd.native import native
    case = next(c for c in CASES if c.name == "fv_body")
    cfg, pop = case.world.config(case.bucket), C.make_pop(case.world, case.batch)
    cpu = _twin(case, cfg, pop)
    cpu.sc.ingest(np.ascontiguousarray(case.steps[0].rows, REQREC).view(np.uint8))
    rows = case.steps[1].rows
    _, feat = cpu.sc.score(np.ascontiguousarray(rows, REQREC).view(np.uint8), case.steps[1].now, False, True)
    lens = [len(native().serialize_feature_vector(f)) for f in np.asarray(feat)]
    for i, row in enumerate(rows):
        s = int(row["slot"])
        if s in C.FV_LENGTHS:
            assert lens[i] == C.FV_LENGTHS[s][0 if int(row["ip_hash"]) == C.IP_C else 1], (i, lens[i])
        if s < 0:
            assert lens[i] == 0
    assert {C.FV_BODY_MAX - 1, C.FV_BODY_MAX, C.FV_BODY_MAX + 1} <= {
        n for n, r in zip(lens, rows) if int(r["tx_type"]) & C.FV_ENC_BIT}
    tags = native().serialize_feature_vector(np.asarray(feat)[0])
    assert b"\x80\x01" in tags                                  # a two-byte tag (field 16, varint)
    assert b"\xff" * 9 + b"\x01" in tags                         # a 10-byte varint (a negative value)


def test_golden_log_transform_against_float64():
    """The f32 golden log_t against float64 log1p at the magnitudes of these cases: the worst
    relative distance measured is 3.4e-8 (the bound: half an f32 ulp, 2^-24 = 5.96e-8), well inside the 2e-7
    the device rows get."""
    worst = 0.0
    vals = [1, 7, 99999, 100000, 100001, 0xFFFFFFFF, 3 * 0xFFFFFFFF + 1, 1 << 40, (1 << 45) - 3, (1 << 45) + (1 << 33)]
    vals += [int(v) for v in np.random.default_rng(0).integers(1, 1 << 46, 2000)]
    for v in vals:
        x = float(np.float32(v))  # the model input is the f32 value
        ref = math.log1p(x)
        worst = max(worst, abs(float(log_t(v, "log1p")) - ref) / ref)
    assert worst <= 2.0 ** -24, worst
