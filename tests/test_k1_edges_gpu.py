"""K1 / K6 edge cases (tests/k1_cases.py), GPU tier: the device kernels against the golden model.

The cases that tests/test_k1_edges.py validates against the C++ twin run here through
``K.feature_update`` (ingest steps), a captured ``GpuScorer`` with the native driver (score steps:
``PipeDriver.set_always_update`` decides between the K1 leader and the update launch) and a
score-only ``GpuScorer`` (probe steps). Scored rows: FeatRec via ``compare_featrec`` plus tx_type,
slot, amount, rule score and reasons; score, action, reasons and ml exact; every row's 128-byte
D2H image is the raw FeatRec or, with FV_ENC_BIT, the host serializer's FeatureVector body.
After every step the store's bytes - tx rings, HLL registers, AcctRT with the cached estimates, GRU event rows - must
equal ``golden_state``. The X rows are compared with ``golden.features.model_input`` at
rtol 2e-7, atol 0 (the bound of test_normalized_inputs_match_golden; the golden log_t itself is
within 3.4e-8 of float64 log1p at these magnitudes, tests/test_k1_edges.py); padded rows of a
bucket come back inert. Paths are selected by construction (k1_cases.expected_path); the
driver's update_skips / update_launches counters are asserted batch by batch.

Stores (64 accounts each) and scorers are built once per world and bucket and reused; every
case starts from a cleared store.
"""
import numpy as np
import pytest

from igaming_platform_amd.layouts import FEATREC, REQREC

from . import k1_cases as C

pytestmark = pytest.mark.gpu

CASES = C.all_cases()
_RIGS = {}
N_ACC = 64    # every store holds 64 accounts; a case uses the first n_acc
_FAULT = []   # a device error of an earlier case: nothing more is launched on that device


class _Rig:
    def __init__(self, world, bucket):
        import torch
        from igaming_platform_amd.engine.scorer import GpuScorer
        from igaming_platform_amd.features.device_store import DeviceFeatureStore
        self.dev = torch.device("cuda", 0)
        self.cfg = world.config(bucket)
        bl, ip = C.make_tables(world)
        self.store = DeviceFeatureStore(N_ACC, self.cfg.features, self.dev, events=True, blacklist=bl, ipintel=ip,
                                        max_events=world.max_events)
        self.store.sync_tables()
        assert self.store.dcap == C.dedup_cap(world.max_events)
        self.probe = GpuScorer(self.cfg, self.store, plan=None, model="heuristic", device=self.dev,
                               update_features=False, use_graphs=False)
        self._scorer = None

    @property
    def scorer(self):
        if self._scorer is None:
            from igaming_platform_amd.engine.scorer import GpuScorer
            g = GpuScorer(self.cfg, self.store, plan=None, model="heuristic", device=self.dev, pipeline_depth=2)
            g.capture()
            assert g.direct and g.driver is not None
            self._scorer = g
        return self._scorer


def _rig(case):
    assert case.n_acc <= N_ACC
    key = (case.world, case.bucket)
    if key not in _RIGS:
        _RIGS[key] = _Rig(*key)
    return _RIGS[key]


def _state(store, n_acc):
    return {k: getattr(store, k)[:n_acc].cpu().numpy() for k in C.STATE_KEYS}


def _check_x(tag, g, n, bucket, want, width):
    X = g.X[:bucket].cpu().numpy()
    for i, w in enumerate(want):
        np.testing.assert_allclose(X[i, :width], w["x"], rtol=2e-7, atol=0, err_msg=f"{tag}: X row {i}")
    assert not X[n:bucket, :width].any(), f"{tag}: padded X rows"
    feat = g.feat[:bucket].cpu().numpy()
    assert (feat[n:, 27] == -1).all() and not np.delete(feat[n:], 27, axis=1).any(), f"{tag}: padded FeatRec rows"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_matches_golden(case):
    if _FAULT:
        pytest.fail("not run: an earlier case ended in a device error: " + _FAULT[0])
    try:
        _run(case)
    except RuntimeError as e:  # HIP errors surface as RuntimeError
        _FAULT.append(f"{case.name}: {e}"[:300])
        raise


def _run(case):
    import torch
    from igaming_platform_amd.native import native
    from igaming_platform_amd.ops import kernels as K
    rig = _rig(case)
    cfg, store = rig.cfg, rig.store
    pop = C.make_pop(case.world, case.batch)
    gold = C.new_golden(case, pop)
    torch.cuda.synchronize()
    store.reset_accounts(np.arange(N_ACC))
    store.set_batch_features(np.arange(case.n_acc), pop.batch)
    store.set_ext(np.arange(case.n_acc), pop.ext)
    width = cfg.features.width
    for q, st in enumerate(case.steps):
        tag = f"{case.name} step {q} ({st.kind})"
        n = len(st.rows)
        if st.kind == "ingest":
            t = torch.from_numpy(np.ascontiguousarray(st.rows, REQREC).view(np.uint8).copy()).to(rig.dev)
            with torch.cuda.stream(rig.probe.stream):
                K.feature_update(store, rig.probe.cfg_dev, t, n, n=n)
            C.apply_rows(gold, pop, st.rows)
        else:
            want = C.golden_rows(cfg, gold, pop, st.rows, st.now)
            g = rig.probe
            if st.kind == "score":
                g = rig.scorer
                g.driver.set_always_update(case.always_update)
                before = (g.driver.update_skips, g.driver.update_launches)
            if st.kind == "score":  # the driver copies the rows and bounds the accounts' multiplicities
                out = g.wait(g.submit_packed(g.next_slot(), n, st.now, want_features=True,
                                             rows=np.ascontiguousarray(st.rows, REQREC)))
            else:
                out = g.score(st.rows, now=st.now, want_features=True)
            torch.cuda.synchronize()
            feats = g.feat[:n].cpu().numpy()   # the device's FeatRec rows; out["features"]: the rows' D2H images
            C.check_scored(tag, st.rows, want, out, feats.view(FEATREC).reshape(-1))
            C.check_images(tag, st.rows, feats, out["features"])
            _check_x(tag, g, n, case.bucket, want, width)
            if st.kind == "score":
                slots = np.ascontiguousarray(st.rows["slot"], np.int32)
                short = native().mult_step_bound(slots, [n]) <= C.k1_seg_max()
                if case.path in ("k1_single", "k1_leader"):
                    assert short, f"{tag}: the driver's bound does not leave the batch to K1"
                skip = short and not case.always_update
                assert (g.driver.update_skips, g.driver.update_launches) == (before[0] + skip, before[1] + (not skip)), tag
                C.apply_rows(gold, pop, st.rows, now=st.now)
        torch.cuda.synchronize()
        d = C.state_diff(_state(store, case.n_acc), C.golden_state(gold, pop, cfg), case.n_acc)
        assert not d, f"{tag}: {d}"
