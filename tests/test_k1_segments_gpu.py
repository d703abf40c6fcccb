"""In a batch whose accounts have at most K1_SEG_MAX events each, the accounts with 2..K1_SEG_MAX
events are scored and applied inside K1, led by the quarter-wave of the account's first row
(csrc/kernels/features.hip feature_assemble_body, AssembleArgs::own_short), and the native driver
launches no multi-event update: the submitter's bound shows that no account needs it (driver.hip,
csrc/include/mult_sketch.h). K1 clears the dedup region of batch seq + DEDUP_AHEAD in every form.

One request stream goes through the CPU engine's scorer (csrc/runtime/cpu_scorer.cpp, sequential
apply) and through two GPU pipelines at depth 3: one that launches the update behind every K1
(PipeDriver.set_always_update) and one where the bound decides. Result rows, FeatRec rows and
the whole feature store (tx rings, HLL registers, AcctRT with the cached estimates, GRU event
rows) must be equal byte for byte between all three. The CPU scorer does not expose its model
input rows, so each batch's X rows are compared, byte for byte, with those of a score-only K1 (no
dedup region: every quarter produces its own row, the path tests/test_kernels_gpu.py holds against
the golden model) run on the CPU scorer's state before the batch.

Every batch has n = 77 live rows in the 128-row bucket (a padded tail and a partly filled wave),
so the issue's multiplicities 1, 2, 3, 15, 16, 17 and 65 (both sides of K1_SEG_MAX and of
DEDUP_LIST) are spread over the batches of the sequence; the same accounts recur in adjacent
batches, over 2 * DEDUP_RING + 4 batches (the region ring wraps twice)."""
import numpy as np
import pytest

from igaming_platform_amd.config import Config

pytestmark = pytest.mark.gpu

NOW = 1_760_000_000
N_ACC = 128
N_LIVE = 77
BUCKET = 128
DEDUP_RING = 8
K1_SEG_MAX = 16

# accounts by role; every other account below N_ACC is a source of single events
A_HOT, A17, A16, A15, A3, A2, A2B = 1, 2, 3, 4, 5, 6, 7
SINGLES = list(range(10, N_ACC))

# batch compositions {account: events}; the rest of the 77 rows: one row without an account
# (slot -1) and single-event accounts
COMP = {
    "fill60": {A16: 60, A3: 3, A2: 2},                      # one wave of the update kernel; ring head -> 60
    "mixed": {A17: 17, A16: 16, A15: 15, A3: 3, A2: 2},     # 17 > K1_SEG_MAX: plain K1 + the update kernel
    "hot": {A_HOT: 65, A3: 3, A2: 2},                       # > DEDUP_LIST: the hot-account workgroups
    "short": {A16: 16, A15: 15, A3: 3, A2: 2, A2B: 2},      # nothing above K1_SEG_MAX: K1 owns them, no update
    "pairs": {A3: 3, A2: 2},                                # mostly single events
}
SEQUENCE = ["fill60", "mixed", "short", "hot", "short", "pairs", "mixed", "short", "short", "hot",
            "pairs", "short", "mixed", "short", "pairs", "short", "hot", "short", "mixed", "short"]
assert len(SEQUENCE) >= 2 * DEDUP_RING + 2


def _hash(hi: int, reg: int) -> int:
    """A 64-bit id digest whose HLL register index is `reg` (low byte) and whose rank comes from `hi`."""
    return ((hi << 8) | reg) & 0xFFFFFFFFFFFFFFFF


# device digests of the multi-event accounts' rows: a repeated hash, two hashes in one HLL word
# (registers 4 and 5 of word 1), two ranks on one register, one blacklisted digest that sits behind
# another key of the same table slot (a probe walk)
DEV_POOL = [_hash(0x00F1E2D3C4B5A6, 4), _hash(0x0000001234567, 5), _hash(0x00F1E2D3C4B5A6, 4),
            _hash(0x000000000ABCD, 4), _hash(0x7A5A5A5A5A5A5A, 200), _hash(0x00000300010002, 77)]
DEV_BLACK = DEV_POOL[5]
DEV_BLACK_FRONT = _hash(0x00000400010002, 77)     # same low 32 bits' table slot (low 16 bits) as DEV_BLACK
IP_POOL = [_hash(0x0000C0A80101, 16), _hash(0x00000A000001, 17), _hash(0x0000C0A80101, 16),
           _hash(0x3FFFFFFFFFFFFF, 19), _hash(0x00000000BEEF01, 130)]
IP_VPN = IP_POOL[4]


def _rows(comp: dict, q: int, pop, rng) -> np.ndarray:
    """77 rows: the composition's accounts dealt round-robin (no two rows of an account K1 owns
    are adjacent, and the rows of the short accounts are spread over the 16-row blocks), one row
    without an account, single-event accounts for the rest."""
    from igaming_platform_amd.utils.synth import make_requests
    n_single = N_LIVE - 1 - sum(comp.values())
    singles = [SINGLES[(11 * q + 3 * i) % len(SINGLES)] for i in range(n_single)]
    assert len(set(singles)) == n_single
    left = dict(comp)
    left.update({s: 1 for s in singles})
    order = sorted(left, key=lambda a: (-left[a], a))
    slots = []
    while left:
        for a in order:
            if a in left:
                slots.append(a)
                left[a] -= 1
                if not left[a]:
                    del left[a]
    slots.insert(5, -1)
    assert len(slots) == N_LIVE
    r = make_requests(pop, N_LIVE, rng, NOW)
    r["slot"] = np.asarray(slots, np.int32)
    seen = {}
    for i, a in enumerate(slots):
        if a in comp:
            k = seen.get(a, 0)
            seen[a] = k + 1
            r["dev_hash"][i] = DEV_POOL[(k * 5 + a + q) % len(DEV_POOL)]
            r["ip_hash"][i] = IP_POOL[(k * 3 + a + 2 * q) % len(IP_POOL)]
    r["ts"] = 0
    return r


def _check_layout(r: np.ndarray, comp: dict) -> bool:
    """The row order the test is about; returns whether a short account has its first row alone
    in a 16-row block (every batch with enough single events beside it has)."""
    slots = r["slot"].tolist()
    assert -1 in slots
    split = False
    for a, c in comp.items():
        rows = [i for i, s in enumerate(slots) if s == a]
        assert len(rows) == c
        if c <= K1_SEG_MAX + 1:
            assert all(b - a_ > 1 for a_, b in zip(rows, rows[1:])), "rows of a short account are adjacent"
        if 2 <= c <= K1_SEG_MAX and all(x // 16 != rows[0] // 16 for x in rows[1:]):
            split = True
    return split


def _world(ring_size: int):
    import torch
    from igaming_platform_amd.engine.backends import NativeCpuBackend
    from igaming_platform_amd.engine.scorer import GpuScorer
    from igaming_platform_amd.features.device_store import DeviceFeatureStore
    from igaming_platform_amd.features.tables import Blacklist, IPIntel
    from igaming_platform_amd.utils.synth import make_population
    dev = torch.device("cuda", 0)
    cfg = Config()
    cfg.features.width = 40
    cfg.features.ring_size = ring_size
    cfg.gpu.buckets = [BUCKET]
    pop = make_population(N_ACC, cfg.features.width - 30, seed=4, fast_hash=True)
    bl, ipi = Blacklist(), IPIntel()
    bl.table.put(DEV_BLACK_FRONT, 0)
    bl.table.put(DEV_BLACK, 0)
    assert bl.table.max_probe >= 2
    ipi.table.put(IP_VPN, IPIntel.VPN)

    def store():
        s = DeviceFeatureStore(N_ACC, cfg.features, dev, events=True, blacklist=bl, ipintel=ipi, max_events=256)
        s.set_batch_features(np.arange(N_ACC), pop.batch)
        s.set_ext(np.arange(N_ACC), pop.ext)
        s.sync_tables()
        return s

    cpu = NativeCpuBackend(cfg, N_ACC, model="heuristic", blacklist=bl, ipintel=ipi)
    cpu.set_batch_rows(np.arange(N_ACC), pop.batch)
    cpu.set_ext(np.arange(N_ACC), pop.ext)
    gpus = []
    for always in (True, False):
        g = GpuScorer(cfg, store(), plan=None, model="heuristic", device=dev, pipeline_depth=3)
        g.capture()
        assert g.direct and g.driver is not None
        g.driver.set_always_update(always)
        gpus.append(g)
    ref = GpuScorer(cfg, store(), plan=None, model="heuristic", device=dev, update_features=False, use_graphs=False)
    return cfg, pop, cpu, gpus, ref


def _load_state(store, st: dict) -> None:
    import torch
    for name, dt in (("ring_ts", np.int32), ("ring_amt", np.int64), ("hll", np.uint8), ("rt", np.int32)):
        t = getattr(store, name)
        t.copy_(torch.from_numpy(np.ascontiguousarray(st[name]).view(dt).reshape(tuple(t.shape)).copy()))


@pytest.mark.parametrize("ring_size", [64, 256])
def test_short_multi_event_accounts_match_cpu_under_both_launch_schedules(ring_size):
    import torch
    from igaming_platform_amd.layouts import ACCTRT, REQREC
    cfg, pop, cpu, gpus, ref = _world(ring_size)
    rng = np.random.default_rng(21)
    batches, split = [], {}
    for q, name in enumerate(SEQUENCE):
        r = _rows(COMP[name], q, pop, rng)
        split[name] = _check_layout(r, COMP[name])
        batches.append((r, NOW + 7 * q))
    assert split["mixed"] and split["short"] and split["pairs"], "no short account's first row is alone in its block"

    # the CPU engine, batch by batch; before each batch its state goes to the score-only K1
    want = []
    for q, (r, now) in enumerate(batches):
        st = cpu.sc.state()
        if q == 1 and ring_size == 64:  # the 16-event account's tx ring wraps in this batch
            rt = np.ascontiguousarray(st["rt"]).view(ACCTRT)
            assert int(rt["ring_head"][A16]) == 60
        _load_state(ref.store, st)
        ref.score(r, now=now)
        x = ref.X[:N_LIVE].cpu().numpy().copy()
        res, feat = cpu.sc.score(np.ascontiguousarray(r, REQREC).view(np.uint8), now, True, True)
        want.append((np.asarray(res).view(np.int32).copy(), np.asarray(feat).view(np.int32).copy(), x))
    final = cpu.sc.state()
    if ring_size == 64:
        rt = np.ascontiguousarray(final["rt"]).view(ACCTRT)
        assert int(rt["ring_head"][A16]) == (60 + 16 * sum(COMP[n].get(A16, 0) == 16 for n in SEQUENCE)) % 64

    # the two GPU pipelines, three batches in flight
    for g in gpus:
        got, inflight = [], []

        def collect(p):
            res, feats = g.wait(p, unpack=False)
            got.append((np.asarray(res).view(np.int32).copy(), np.asarray(feats).view(np.int32).copy(),
                        g.slots[p.slot].X[:N_LIVE].cpu().numpy().copy()))

        for r, now in batches:
            inflight.append(g.submit_packed(g.next_slot(), N_LIVE, now, want_features=True, rows=r))
            if len(inflight) == 3:
                collect(inflight.pop(0))
        for p in inflight:
            collect(p)
        torch.cuda.synchronize()
        always = g.driver.always_update
        for q, ((res, feat, x), (wres, wfeat, wx)) in enumerate(zip(got, want)):
            tag = f"batch {q} ({SEQUENCE[q]}), update {'always' if always else 'by bound'}"
            np.testing.assert_array_equal(res.reshape(-1, 2), wres.reshape(-1, 2), err_msg="results, " + tag)
            np.testing.assert_array_equal(feat.reshape(-1, 32), wfeat.reshape(-1, 32), err_msg="FeatRec, " + tag)
            assert x.tobytes() == wx.tobytes(), "X rows, " + tag
        s = g.store
        for name in ("ring_ts", "ring_amt", "hll", "rt", "ev"):
            have = getattr(s, name).cpu().numpy().tobytes()
            assert have == np.ascontiguousarray(final[name]).tobytes(), (name, "always" if always else "by bound")
        if always:
            assert g.driver.update_skips == 0 and g.driver.update_launches == len(SEQUENCE)
        else:  # batches on both sides of the bound
            assert g.driver.update_skips >= SEQUENCE.count("pairs")
            assert g.driver.update_launches >= len(SEQUENCE) - SEQUENCE.count("pairs") - SEQUENCE.count("short")
            assert g.driver.update_skips + g.driver.update_launches == len(SEQUENCE)
            assert g.driver.update_skips > 0 and g.driver.update_launches > 0
