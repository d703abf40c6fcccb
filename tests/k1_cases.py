"""Case tables and the reference for the K1 / K6 edge suite (no torch, no GPU).

K1 (feature assembly: window counts and sums over the tx ring, TTL reads, cached HLL counts, the
blacklist / IP-intel probes, the rule pass, the model-input row) and every K6 write path
(csrc/kernels/features.hip) are held against ``igaming_platform_amd.golden`` - exact integer
arithmetic in Python. Every case is a tiny world (at most 64 accounts) and a list of steps:

  ``ingest``  standalone ordered ingestion of events that carry their own ``ts``
              (``K.feature_update`` / ``CpuScorer.ingest`` / ``gold.apply`` in row order),
  ``score``   a score-then-update batch at one clock,
  ``probe``   a score-only batch (the state is left alone; one state is probed at many clocks).

tests/test_k1_edges.py runs the cases through the golden model and the C++ twin (CpuScorer),
tests/test_k1_edges_gpu.py through the device kernels; both compare the scored rows and, after
every step, every byte of the store with :func:`golden_state`.

Write paths, named by who applies an account's events (:func:`expected_path`):

  k1_single          apply_event_q: the account's only event of a scoring batch, inside K1
  k1_leader          apply_list_segment from K1: 2..K1_SEG_MAX events, no account of the batch above
  seg_list           update_segments_kernel, 2..DEDUP_LIST events
  seg_hot            update_hot_body, more than DEDUP_LIST events
  ing_single         update_single_kernel
  ing_list_parallel  update_multi_kernel -> apply_chunk, span < min TTL
  ing_list_serial    update_multi_kernel -> apply_chunk, span >= min TTL
  ing_scan           apply_scan_chunks, more than DEDUP_LIST events

Cells of the path x edge matrix left out on purpose are listed in ``LEFT_OUT`` with the reason.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from igaming_platform_amd.config import Config, REASON_BIT
from igaming_platform_amd.features.device_store import DEDUP_LIST
from igaming_platform_amd.golden import hll as GH
from igaming_platform_amd.golden import scoring as GS
from igaming_platform_amd.golden.features import GoldenFeatureStore, TxEvent, model_input
from igaming_platform_amd.layouts import ACCTBATCH, ACCTRT, REQREC
from igaming_platform_amd.utils.synth import Population

from .helpers import compare_featrec

NOW = 1_760_000_000
HOT_TAIL_MAX = 192      # csrc/kernels/features.hip: the hot workgroup's exact tail, in events
MAX_EVENTS = 1024       # the stores' dedup capacity (rows per ingest call / scoring batch)
FV_ENC_BIT = 1 << 16    # csrc/include/records.h: ReqRec.tx_type bit, the row's image is the encoded FeatureVector body
FV_BODY_MAX = 126       # a longer body leaves the raw FeatRec as the row's image (byte 127 clear)

PATHS = ("k1_single", "k1_leader", "seg_list", "seg_hot",
         "ing_single", "ing_list_parallel", "ing_list_serial", "ing_scan")
SCORE_PATHS, INGEST_PATHS = PATHS[:4], PATHS[4:]
SMALL_TTL = dict(session_ttl_s=700, sum_ttl_s=500, hll_ttl_s=900, last_tx_ttl_s=1300)  # the sum's is the minimum


def k1_seg_max() -> int:
    from igaming_platform_amd.native import native
    return int(native().K1_SEG_MAX)


# ------------------------------------------------------------------------------------ worlds
@dataclass(frozen=True)
class World:
    ring: int = 256
    ev_ring: int = 100
    width: int = 30
    ttl: str = "default"      # "small": SMALL_TTL
    sum_mode: str = "sliding"
    log: str = "log1p"
    tables: str = ""          # key of TABLES
    max_events: int = MAX_EVENTS
    review: int = 50          # ScoringConfig.review_threshold / block_threshold
    block: int = 80

    def config(self, bucket: int = 64) -> Config:
        cfg = Config()
        f = cfg.features
        f.ring_size, f.event_ring, f.width = self.ring, self.ev_ring, self.width
        f.sum_mode, f.log_transform = self.sum_mode, self.log
        if self.ttl == "small":
            for k, v in SMALL_TTL.items():
                setattr(f, k, v)
        cfg.scoring.review_threshold, cfg.scoring.block_threshold = self.review, self.block
        cfg.gpu.buckets = [bucket]
        cfg.gpu.max_batch = bucket
        cfg.validate()
        return cfg

    def ttls(self) -> Dict[str, int]:
        f = self.config().features
        return dict(session=f.session_ttl_s, sum=f.sum_ttl_s, hll_dev=f.hll_ttl_s, hll_ip=f.hll_ttl_s,
                    last_tx=f.last_tx_ttl_s)

    def min_ttl(self) -> int:
        return min(self.ttls().values())


@dataclass
class Step:
    kind: str                 # ingest | score | probe
    rows: np.ndarray          # REQREC
    now: int = 0
    setup: bool = False       # state from before the edge (never the visit that selects the path)


@dataclass
class Case:
    name: str
    world: World
    batch: np.ndarray         # ACCTBATCH [n_acc]
    steps: List[Step]
    bucket: int = 64
    path: str = ""            # write cases: the path under test ...
    edge: str = ""            # ... and the edge it meets
    focus: int = 0            # the account whose events select the path
    always_update: bool = False   # scorer path: the update launch behind every K1 (PipeDriver.set_always_update)
    visits: Tuple[Tuple[int, int, int], ...] = ()   # (slot, clock, events): each lies whole in one step of that clock
    chosen: Tuple[Tuple[int, int, int, int], ...] = ()  # (slot, first rank, last rank, events) of the chosen events

    @property
    def n_acc(self) -> int:
        return len(self.batch)


# ------------------------------------------------------------------------------------ helpers
def mix32(x: int) -> int:
    """csrc/kernels/update.h mix32: an account slot's home in a dedup region is mix32(slot) & (cap - 1)."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def dedup_cap(max_events: int) -> int:
    c = 1
    while c < 2 * max_events:
        c <<= 1
    return c


def colliding_slots(max_events: int, n_acc: int = 64) -> Tuple[int, int]:
    """Two account slots with the same home slot in a dedup region of a store with ``max_events``."""
    cap, seen = dedup_cap(max_events), {}
    for s in range(n_acc):
        h = mix32(s) & (cap - 1)
        if h in seen:
            return seen[h], s
        seen[h] = s
    raise AssertionError("no two slots share a home slot")


def hash_for(reg: int, rank: int, salt: int = 0) -> int:
    """A 64-bit id digest that lands on HLL register ``reg`` with rank ``rank`` (1..57; 57: h >> 8 == 0,
    which for register 0 is hash 0 - no PFADD at all)."""
    assert 0 <= reg < 256 and 1 <= rank <= 57
    if rank == 57:
        return reg
    top = 56 - rank
    return ((((1 << top) | (salt & ((1 << top) - 1))) << 8) | reg) & 0xFFFFFFFFFFFFFFFF


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round to nearest even (common.h f32_to_bf16; no NaN here)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


class CountingGolden(GoldenFeatureStore):
    """The golden store, which also counts each account's events (the GRU ring's head)."""

    def __init__(self, cfg=None):
        super().__init__(cfg)
        self.n_events: Dict[str, int] = {}

    def apply(self, ev) -> None:
        super().apply(ev)
        self.n_events[ev.account] = self.n_events.get(ev.account, 0) + 1


def golden_state(gold: CountingGolden, pop: Population, cfg: Config) -> Dict[str, np.ndarray]:
    """The golden store in the device layout: ring_ts / ring_amt [n, R], hll [n, 512] (device file,
    then ip file), rt (layouts.ACCTRT [n]; the cached hll_*_n = hll.count of the registers, pad 0)
    and ev (bf16 bit patterns [n, event_ring, event_dim], rows at their ring positions)."""
    f = cfg.features
    n, R, E, D = len(pop.ids), f.ring_size, f.event_ring, f.event_dim
    ring_ts = np.zeros((n, R), np.uint32)
    ring_amt = np.zeros((n, R), np.int64)
    regs = np.zeros((n, 512), np.uint8)
    rt = np.zeros(n, ACCTRT)
    ev = np.zeros((n, E, D), np.uint16)
    for i, aid in enumerate(pop.ids):
        st = gold.accounts.get(aid)
        if st is None:
            continue
        ring_ts[i] = np.asarray(st.ring_ts, np.int64).astype(np.uint32)
        ring_amt[i] = st.ring_amt
        regs[i, :256] = np.frombuffer(bytes(st.hll_dev), np.uint8)
        regs[i, 256:] = np.frombuffer(bytes(st.hll_ip), np.uint8)
        r = rt[i]
        r["hll_dev_exp"], r["hll_ip_exp"] = st.hll_dev_exp, st.hll_ip_exp
        r["last_tx"], r["last_tx_exp"] = st.last_tx, st.last_tx_exp
        r["session_start"], r["session_exp"] = st.session_start, st.session_exp
        r["sum_exp"], r["sum_compat"] = st.sum_compat_exp, st.sum_compat
        r["last_event_ts"] = st.last_event_ts
        r["ring_head"] = st.head
        tot = gold.n_events.get(aid, 0)
        assert len(st.events) == min(tot, E)
        r["ev_head"], r["ev_count"] = tot % E, min(tot, E)
        r["hll_dev_n"], r["hll_ip_n"] = GH.count(st.hll_dev), GH.count(st.hll_ip)
        for j, row in enumerate(st.events):
            ev[i, (tot - len(st.events) + j) % E] = bf16_bits(row)
    return dict(ring_ts=ring_ts, ring_amt=ring_amt, hll=regs, rt=rt, ev=ev)


STATE_KEYS = ("ring_ts", "ring_amt", "hll", "rt", "ev")


def state_diff(have: Dict[str, np.ndarray], want: Dict[str, np.ndarray], n_acc: int) -> str:
    """"" when ``have`` equals ``want`` byte for byte; else which array and account differ first."""
    for k in STATE_KEYS:
        h = np.ascontiguousarray(have[k]).view(np.uint8).reshape(n_acc, -1)
        w = np.ascontiguousarray(want[k]).view(np.uint8).reshape(n_acc, -1)
        if h.shape != w.shape:
            return f"{k}: {h.shape[1]} bytes per account, golden {w.shape[1]}"
        bad = np.nonzero((h != w).any(axis=1))[0]
        if len(bad):
            a = int(bad[0])
            if k == "rt":
                hr, wr = h[a].view(ACCTRT)[0], w[a].view(ACCTRT)[0]
                d = {n: (int(hr[n]), int(wr[n])) for n in ACCTRT.names if n != "pad" and hr[n] != wr[n]}
                return f"rt of account {a}: (have, golden) {d}"
            o = int(np.nonzero(h[a] != w[a])[0][0])
            return f"{k} of account {a}: first difference at byte {o} ({len(bad)} accounts differ)"
    return ""


def apply_rows(gold: CountingGolden, pop: Population, rows: np.ndarray, now: Optional[int] = None) -> None:
    """The rows' events in row order; ``now``: a scoring batch, every event at the batch clock."""
    for r in rows:
        if int(r["slot"]) >= 0:
            gold.apply(TxEvent(pop.ids[int(r["slot"])], int(r["amount"]), int(r["tx_type"]) & 0xFF, int(r["dev_hash"]),
                               int(r["ip_hash"]), int(r["ts"]) if now is None else now))


def golden_rows(cfg: Config, gold: CountingGolden, pop: Population, rows: np.ndarray, now: int) -> List[dict]:
    """helpers.golden_score of every row (heuristic model); an account's state is read once per batch."""
    cache: Dict[int, dict] = {}
    out = []
    for row in rows:
        s = int(row["slot"])
        aid = pop.ids[s] if s >= 0 else "__unknown__"
        if s not in cache:
            cache[s] = gold.raw_features(aid, now, ip_hash=0)
        f = dict(cache[s])
        fl = gold.ip_intel.get(int(row["ip_hash"]), 0) if int(row["ip_hash"]) else 0
        f["is_vpn"], f["is_proxy"], f["is_tor"] = bool(fl & 1), bool(fl & 2), bool(fl & 4)
        if s < 0:
            f["_partial"] = True
        bl = gold.blacklisted([int(row["dev_hash"]), int(row["fp_hash"]), int(row["ip_hash"])], now)
        amount, tx = int(row["amount"]), int(row["tx_type"]) & 0xFF
        rule, rule_reasons = GS.apply_rules(cfg.scoring, f, amount, tx, bl)
        ext = gold.accounts[aid].ext if (s >= 0 and aid in gold.accounts) else None
        x = model_input(f, amount, tx, cfg.features.log_transform, cfg.features.width, ext)
        score, action, reasons, ml = GS.ensemble(cfg.scoring, rule, rule_reasons, GS.heuristic_predict(x))
        out.append(dict(features=f, blacklisted=bl, rule=rule, rule_reasons=rule_reasons, reasons=reasons,
                        score=score, action=action, ml=ml, x=x))
    return out


def _mask(reasons) -> int:
    return sum(1 << REASON_BIT[r] for r in reasons)


def check_scored(tag: str, rows: np.ndarray, want: List[dict], out: dict, feats: np.ndarray) -> None:
    """Result rows (layouts.unpack_results) and FeatRec rows against the golden rows: every integer,
    flag and f32 field exact."""
    for i, (row, g) in enumerate(zip(rows, want)):
        t = f"{tag}, row {i} (slot {int(row['slot'])})"
        try:
            compare_featrec(feats[i], g, i)
        except AssertionError as e:
            raise AssertionError(f"{t}: {e}") from None
        fr = feats[i]
        assert (int(fr["tx_type"]), int(fr["slot"]), int(fr["amount"])) == (
            int(row["tx_type"]) & 0xFF, int(row["slot"]), int(row["amount"])), t
        assert int(fr["rule_score"]) == g["rule"] and int(fr["rule_reasons"]) == _mask(g["rule_reasons"]), (
            t, int(fr["rule_score"]), g["rule"], int(fr["rule_reasons"]), g["rule_reasons"])
        assert int(out["score"][i]) == g["score"] and int(out["action"][i]) == g["action"], (
            t, int(out["score"][i]), g["score"])
        assert int(out["rule_score"][i]) == g["rule"], t
        assert int(out["reasons"][i]) == _mask(g["reasons"]), (t, int(out["reasons"][i]), g["reasons"])
        assert np.float32(out["ml"][i]) == np.float32(g["ml"]), (t, out["ml"][i], g["ml"])


def check_images(tag: str, rows: np.ndarray, feats: np.ndarray, images: np.ndarray) -> None:
    """The rows' 128-byte D2H images against their FeatRec rows (int32 [n, 32] each): a row with
    FV_ENC_BIT whose FeatureVector body (the host serializer's bytes) fits 126 bytes carries that
    body and byte 127 = 0x80 | length; every other row's image is the raw FeatRec, byte 127 clear."""
    from igaming_platform_amd.native import native
    ser = native().serialize_feature_vector
    feats = np.ascontiguousarray(feats).view(np.int32).reshape(len(rows), 32)
    img = np.ascontiguousarray(images).view(np.uint8).reshape(len(rows), 128)
    for i, row in enumerate(rows):
        body = ser(feats[i])
        if int(row["tx_type"]) & FV_ENC_BIT and len(body) <= FV_BODY_MAX:
            assert int(img[i, 127]) == 0x80 | len(body), (tag, i, int(img[i, 127]), len(body))
            assert img[i, :len(body)].tobytes() == body, f"{tag}: encoded body of row {i} ({len(body)} bytes)"
        else:
            assert img[i].tobytes() == feats[i].tobytes() and img[i, 127] == 0, f"{tag}: raw image of row {i}"


def make_pop(world: World, batch: np.ndarray) -> Population:
    n, w = len(batch), world.width - 30
    ext = (((np.arange(n)[:, None] * 131 + np.arange(max(w, 0))[None, :] * 17) % 97) / 97.0).astype(np.float32)
    z = np.zeros((n, 1), np.uint64)
    return Population([f"acct-{i:04d}" for i in range(n)], np.ascontiguousarray(batch, ACCTBATCH), ext, z, z, z)


def new_golden(case: Case, pop: Population) -> CountingGolden:
    cfg = case.world.config(case.bucket)
    gold = CountingGolden(cfg.features)
    for i, aid in enumerate(pop.ids):
        gold.set_batch(aid, pop.golden_batch(i))
        gold.set_ext(aid, pop.ext[i] if case.world.width > 30 else None)
    bl, ip = TABLES[case.world.tables]
    gold.blacklist.update({k: e for k, e in bl})
    gold.ip_intel.update({k: v for k, v in ip})
    return gold


def make_tables(world: World):
    """The world's Blacklist / IPIntel (features.tables), the smallest tables (16 slots)."""
    from igaming_platform_amd.features.tables import Blacklist, IPIntel
    bl, ip = Blacklist(16), IPIntel(16)
    for k, e in TABLES[world.tables][0]:
        bl.table.put(k, e)
    for k, v in TABLES[world.tables][1]:
        ip.table.put(k, v)
    return bl, ip


def default_batch(n: int, now: int = NOW) -> np.ndarray:
    b = np.zeros(n, ACCTBATCH)
    i = np.arange(n)
    b["total_deposits"] = 20000 + 997 * i
    b["total_withdrawals"] = 3000 + 101 * i
    b["deposit_count"], b["withdraw_count"] = 3 + i % 4, i % 3
    b["bet_count"], b["win_count"] = 10 + i, 3 + i // 2
    b["total_bets"], b["total_wins"] = 5000 + 11 * i, 4000 + 7 * i
    b["avg_bet_size"] = (b["total_bets"] / b["bet_count"]).astype(np.float32)
    b["account_created_at"] = now - 86400 * (30 + i) - 17 * i
    b["bonus_claim_count"] = i % 3
    b["bonus_wager_complete"] = ((i % 10) / 10.0).astype(np.float32)
    b["present"] = 1
    return b


def rows_of(items) -> np.ndarray:
    """REQREC rows from (slot, ts, amount, tx_type, dev, ip[, fp]) tuples."""
    r = np.zeros(len(items), REQREC)
    for i, it in enumerate(items):
        r["slot"][i], r["ts"][i], r["amount"][i], r["tx_type"][i] = it[0], it[1], it[2], it[3]
        r["dev_hash"][i], r["ip_hash"][i] = it[4], it[5]
        r["fp_hash"][i] = it[6] if len(it) > 6 else 0
    return r


def interleave(per_slot: List[np.ndarray]) -> np.ndarray:
    """Round-robin merge: every account's rows keep their order, rows of one account are apart."""
    per_slot = [r for r in per_slot if len(r)]
    out, k = [], 0
    while any(k < len(r) for r in per_slot):
        out += [r[k:k + 1] for r in per_slot if k < len(r)]
        k += 1
    return np.concatenate(out) if out else np.zeros(0, REQREC)


DEV0, DEV1 = hash_for(10, 3, 0x5151), hash_for(11, 9, 0x77)
IP0, IP1 = hash_for(200, 2, 0x1234), hash_for(201, 6, 0x99)
AMOUNTS = [0, -7, 99999, 100000, 100001, 1 << 40]


def probe_rows(slots, now: int, keys: Optional[Callable[[int], tuple]] = None) -> np.ndarray:
    """Score-only rows: amounts on both sides of the large-amount rule, every tx type (0..7)."""
    items = []
    for i, s in enumerate(slots):
        dev, fp, ip = keys(i) if keys else (0, 0, 0)
        items.append((s, now, AMOUNTS[i % len(AMOUNTS)], i % 8, dev, ip, fp))
    return rows_of(items)


# ------------------------------------------------------------------------------------ tables
# 16-slot tables (home slot = low 4 bits of the key's low 32 bits).
def _k(home: int, tag: int, high: int = 0) -> int:
    return (high << 32) | (tag << 4) | home


BL_A, BL_B, BL_C, BL_D = _k(15, 1), _k(15, 2), _k(15, 3), _k(15, 4)   # one chain: slots 15, 0, 1, 2
BL_ABSENT = _k(15, 5)                       # walks the whole chain (max_probe keys) and is not there
BL_HIGH, BL_HIGH_OTHER = _k(5, 7, high=7), _k(5, 7, high=9)   # equal low 32 bits
BOTH = _k(7, 9)                             # one ip in both tables
IP_A, IP_B, IP_C = _k(15, 11), _k(15, 12), _k(15, 13)       # chain: slots 15, 0, 1
IP_T = _k(3, 14)                            # Tor only
TABLES = {
    "": ([], []),
    # expiry 0: never; NOW: no longer listed at NOW; NOW + 1: listed at NOW, not at NOW + 1
    "edges": ([(BL_A, 0), (BL_B, NOW + 1), (BL_C, NOW), (BL_D, 0), (BL_HIGH, 0), (BOTH, 0)],
              [(IP_A, 1), (IP_B, 2), (IP_C, 5), (BOTH, 2), (IP_T, 4)]),
}
TABLE_KEYS = [  # (device, fingerprint, ip) of a probe row
    (BL_A, 0, 0), (0, BL_A, 0), (0, 0, BL_A),            # a hit through each position, the others zero
    (BL_B, 0, 0), (BL_C, 0, 0),                           # expiries NOW + 1 and NOW
    (BL_D, 0, 0), (0, 0, BL_D),                           # found on the last allowed probe
    (BL_ABSENT, BL_ABSENT, BL_ABSENT),                    # a chain of max_probe other keys
    (BL_HIGH, 0, 0), (BL_HIGH_OTHER, 0, 0), (BL_A | (3 << 32), 0, 0),
    (0, 0, BOTH), (0, 0, IP_A), (0, 0, IP_B), (0, 0, IP_C), (IP_C, IP_A, 0),   # ip keys are no blacklist keys
    (BL_ABSENT, BL_C, IP_C), (0, 0, 0),
]


# ------------------------------------------------------------------------------------ read path
EDGE_ENTRIES = [(NOW - 59, 0xFFFFFFFF), (NOW - 60, 0xFFFFFFFF), (NOW - 61, 1), (NOW - 300, -5), (NOW - 301, 0),
                (NOW - 3600, (1 << 45) - 3), (NOW - 3601, 0xFFFFFFFF), (NOW + 5, 0xFFFFFFFF)]
READ_WORLDS = [World(64, 100, 30), World(128, 100, 32, sum_mode="compat"), World(192, 100, 33),
               World(256, 100, 142), World(320, 100, 143, sum_mode="compat", log="identity"), World(512, 100, 160)]
N_LIVE = (63, 17, 16, 15, 1)
A_NEVER, A_TTL = 24, 25


def ring_positions(R: int) -> List[int]:
    return sorted({0, 1, 2, 3, 63, R - 1} | ({64} if R > 64 else set()) | ({255, 256} if R > 256 else set()))


def _filler(m: int):
    return (NOW - 7200 - m % 1000, 1000 + m)   # outside the hour, not empty


def window_case(w: World) -> Case:
    """Accounts 0-7: a full ring (head back at 0), entry set rotated over the chosen positions;
    8-15: the same after a wrap (R + 37 events); 16-23: four events only (positions 0-3, the
    amount pairs {0,1} / {2,3} with one entry inside the hour and one outside, both orders), all
    other entries empty; 24: never an event; 25: one event (the TTL reads). A ring that is empty
    but for entries at positions 63, 64, 255, 256 or R - 1 cannot be built through the public paths
    (they fill a ring from its head): READ_LEFT_OUT."""
    R, P = w.ring, ring_positions(w.ring)
    steps = []

    def final(k):
        f = [_filler(m) for m in range(R)]
        for i, p in enumerate(P):
            f[p] = EDGE_ENTRIES[(i + k) % 8]
        return f

    for k in range(8):
        f = final(k)
        steps.append(Step("ingest", rows_of([(k, t, a, 2, 0, 0) for t, a in f])))
        ev = [(NOW - 10 - m, 5) for m in range(37)] + [f[m % R] for m in range(37, R + 37)]
        steps.append(Step("ingest", rows_of([(8 + k, t, a, 2, 0, 0) for t, a in ev])))
        four = [EDGE_ENTRIES[(i + k) % 8] for i in range(4)]
        steps.append(Step("ingest", rows_of([(16 + k, t, a, 2, 0, 0) for t, a in four])))
    t0 = NOW - 50
    steps.append(Step("ingest", rows_of([(A_TTL, t0, 1234, 0, DEV0, IP0)])))
    slots = [A_TTL, -1, A_NEVER] + list(range(24))
    clocks = [(NOW, 63), (NOW + 1, 17), (NOW - 1, 16), (NOW + 2, 15), (NOW + 60, 1)]
    for ttl in sorted(set(w.ttls().values())):
        clocks += [(t0 + ttl - 1, len(slots)), (t0 + ttl, len(slots))]
    for now, n in clocks:
        steps.append(Step("probe", probe_rows([slots[i % len(slots)] for i in range(n)], now), now))
    return Case(f"windows_r{R}_w{w.width}_{w.sum_mode}", w, default_batch(26), steps, bucket=64, edge="windows")


RULE_SCORES = (36, 97)   # two final scores the rules case reaches (asserted in tests/test_k1_edges.py)


def rules_case(review: int = 50, block: int = 80) -> Case:
    """Batch features and the rule pass, each threshold at the threshold and one past it. The review /
    block thresholds are met by moving them: onto two scores the case reaches, and one past them."""
    from igaming_platform_amd.config import ScoringConfig
    sc = ScoringConfig()
    day = 86400
    b = default_batch(40)
    steps: List[Step] = []
    ing = []
    # 0-5: account age (truncation toward zero; both sides of new_account_days)
    for i, c in enumerate([NOW + 1, NOW + day - 1, NOW + day, NOW - sc.new_account_days * day + 1,
                           NOW - sc.new_account_days * day, NOW - sc.new_account_days * day - 1]):
        b["account_created_at"][i] = c
    b["present"][6] = 0                                   # 6: partial
    b["bet_count"][7] = 0                                 # 7: no win rate
    for i, (claims, dep) in enumerate([(3, 4999), (4, 4999), (4, 5000), (3, 5000)]):   # 8-11: bonus-only player
        b["bonus_claim_count"][8 + i], b["total_deposits"][8 + i] = claims, dep
    for i, cnt in enumerate([sc.max_tx_per_minute, sc.max_tx_per_minute + 1]):         # 12-13: velocity
        ing += [(12 + i, NOW - 60 + j, 10, 2, 0, 0) for j in range(cnt)]
    for i, cnt in enumerate([sc.max_devices_per_day, sc.max_devices_per_day + 1]):     # 14-15: devices
        ing += [(14 + i, NOW - 500, 10, 2, hash_for(20 + j, 4, j), 0) for j in range(cnt)]
    for i, cnt in enumerate([sc.max_ips_per_day, sc.max_ips_per_day + 1]):             # 16-17: ips
        ing += [(16 + i, NOW - 500, 10, 2, 0, hash_for(40 + j, 4, j)) for j in range(cnt)]
    # 18-27: rapid deposit -> withdraw: last tx 299 / 300 s ago, an expired last tx (the field reads 0),
    # withdrawals on both sides of deposits * 80 / 100 where the integer division matters, no deposits
    rapid = [(299, 101, 81, 2), (300, 101, 81, 2), (299, 101, 80, 2), (299, 104, 83, 2), (299, 104, 84, 2),
             (7 * day, 101, 81, 2), (7 * day + 1, 101, 81, 2), (299, 101, 81, 0), (299, -101, -80, 2),
             (299, -101, -81, 2)]
    for i, (ago, dep, wd, cnt) in enumerate(rapid):
        s = 18 + i
        b["total_deposits"][s], b["total_withdrawals"][s], b["deposit_count"][s] = dep, wd, cnt
        ing.append((s, NOW - ago, 10, 0, 0, 0))
    # 28: every rule the account's state can give at once: the sum clips at 100
    b["account_created_at"][28] = NOW - 5
    b["bonus_claim_count"][28], b["total_deposits"][28], b["total_withdrawals"][28] = 9, 100, 90
    b["deposit_count"][28] = 1
    ing += [(28, NOW - 30 + j, 10, 2, hash_for(60 + j, 4, j), hash_for(80 + j, 4, j)) for j in range(12)]
    # 29-30: ml_high_risk_threshold. The heuristic model adds its terms in float64 in a fixed order:
    # velocity 0.2 + devices 0.15 + ips 0.1 + Tor 0.25 is exactly 0.7 (not above: no ML_HIGH_RISK), and
    # velocity 0.2 + ips 0.1 + VPN 0.15 + Tor 0.25 is 0.7000000000000001, one ulp past it
    for s, ndev in ((29, sc.max_devices_per_day + 1), (30, 0)):
        ing += [(s, NOW - 40 + j, 10, 2, hash_for(110 + j, 4, j) if j < ndev else 0,
                 hash_for(130 + j % (sc.max_ips_per_day + 1), 4, j)) for j in range(sc.max_tx_per_minute + 1)]
    steps.append(Step("ingest", rows_of(sorted(ing, key=lambda t: t[0]))))
    reqs = [(100000, 0), (100001, 0), (500, 1), (100001, 1)]
    for now in (NOW, NOW + 1):
        # account 28's requests also come from a blacklisted device over a VPN address
        items = [(s, now, a, t, BL_A if s == 28 else 0, IP_A if s == 28 else 0) for s in range(29) for a, t in reqs]
        items += [(29, now, 500, 0, 0, IP_T), (30, now, 500, 0, 0, IP_C), (29, now, 500, 0, 0, 0)]
        steps.append(Step("probe", rows_of(items), now))
    return Case(f"rules_review{review}_block{block}", World(tables="edges", review=review, block=block), b, steps,
                bucket=128, edge="rules")


def tables_case() -> Case:
    """Blacklist / IP-intel probes: the walk's wrap to slot 0, the last allowed probe, a full chain
    without the key, keys equal in their low 32 bits, the expiries, a zero hash in each position."""
    steps = []
    for now in (NOW - 1, NOW, NOW + 1):
        slots = [0, -1, 1] * 6
        steps.append(Step("probe", probe_rows(slots, now, keys=lambda i: TABLE_KEYS[i % len(TABLE_KEYS)]), now))
    return Case("tables", World(width=33, tables="edges"), default_batch(4), steps, bucket=64, edge="tables")


# FeatureVector bodies: accounts 0-2 differ only in total_withdrawals (a 1-, 2- and 3-byte varint), so
# that with the VPN + Tor flags of IP_C their bodies are 125, 126 and 127 bytes long (host serializer;
# asserted in tests/test_k1_edges.py): negative totals, counts and age (10-byte varints), two-byte
# tags for fields 16-26. Without the flags (6 bytes less) all three fit. The longest reachable body
# (every int field negative, all three ip flags) is 145 bytes, so rows above the limit exist.
FV_ACCOUNTS = {0: 3, 1: 200, 2: 20000}          # slot -> total_withdrawals
FV_LENGTHS = {0: (125, 119), 1: (126, 120), 2: (127, 121)}   # slot -> body bytes (with IP_C, without)


def fv_case() -> Case:
    b = default_batch(8)
    for s, wd in FV_ACCOUNTS.items():
        b["total_deposits"][s], b["total_withdrawals"][s] = -1000, wd
        b["deposit_count"][s] = b["withdraw_count"][s] = b["bonus_claim_count"][s] = -1
        b["account_created_at"][s] = NOW + 3 * 86400 + 5
        b["bet_count"][s], b["win_count"][s], b["avg_bet_size"][s], b["bonus_wager_complete"][s] = 4, 2, 1.5, 0.5
    b["present"][7] = 0
    ing = [(s, NOW - 10, -5, 2, DEV0, IP0) for s in FV_ACCOUNTS] + [(5, NOW - 70, 1 << 33, 0, DEV0, IP1)]
    steps = [Step("ingest", rows_of(ing))]
    items = []
    for i, s in enumerate([0, 1, 2, 0, 1, 2, 3, 4, 5, 6, 7, -1, 0, 1, 2]):
        ip = IP_C if i < 3 else IP_A if i in (6, 7) else 0
        enc = 0 if i >= 12 else FV_ENC_BIT      # the last three: the same accounts without the bit
        items.append((s, NOW, AMOUNTS[i % len(AMOUNTS)], (i % 6) | enc, BL_A if i == 8 else 0, ip))
    steps.append(Step("probe", rows_of(items), NOW))
    return Case("fv_body", World(tables="edges"), b, steps, bucket=64, edge="fv")


def read_cases() -> List[Case]:
    lo, hi = RULE_SCORES
    return [window_case(w) for w in READ_WORLDS] + [rules_case(), rules_case(lo, hi), rules_case(lo + 1, hi + 1),
                                                   tables_case(), fv_case()]


# ------------------------------------------------------------------------------------ write paths
PATH_K = {"k1_single": 1, "k1_leader": 3, "seg_list": 20, "seg_hot": 150,
          "ing_single": 1, "ing_list_parallel": 5, "ing_list_serial": 5, "ing_scan": 70}


def event(amount=250, tx_type=2, dev=DEV0, ip=IP0, fp=0) -> dict:
    return dict(amount=amount, tx_type=tx_type, dev=dev, ip=ip, fp=fp)


def event_times(path: str, clock: int, k: int, min_ttl: int) -> List[int]:
    """The ts of a visit's k events: the first at ``clock``. Scorer paths: all at the batch clock.
    ing_list_parallel / ing_scan: one second apart. ing_list_serial: the rest at least min_ttl later."""
    if path in SCORE_PATHS or k == 1:
        return [clock] * k
    if path == "ing_list_serial":
        return [clock] + [clock + min_ttl + j - 1 for j in range(1, k)]
    return [clock + j for j in range(k)]


def visit(path: str, slot: int, clock: int, events: List[dict], min_ttl: int) -> np.ndarray:
    ts = event_times(path, clock, len(events), min_ttl)
    return rows_of([(slot, t, e["amount"], e["tx_type"], e["dev"], e["ip"], e["fp"]) for t, e in zip(ts, events)])


def padded(path: str, events: List[dict], tail: bool = True, k: Optional[int] = None) -> List[dict]:
    """``events`` brought to the path's multiplicity by repeating a plain event in front of them
    (tail: the chosen events are the last, applied with exact semantics) or behind them."""
    k = max(k or PATH_K[path], len(events))
    pad = [event(amount=40 + j, tx_type=j % 4) for j in range(k - len(events))]
    return pad + events if tail else events + pad


class Builder:
    """Steps of a write case: visits grouped by clock; on the ingestion paths a score-only probe of
    every account goes in front of each step (the read at the same clock the events arrive at)."""

    def __init__(self, path: str, world: World, n_acc: int):
        self.path, self.world, self.n_acc = path, world, n_acc
        self.min_ttl = world.min_ttl()
        self.visits: Dict[int, List[np.ndarray]] = {}
        self.steps: List[Step] = []
        self.last: Dict[int, int] = {}
        self.log: List[Tuple[int, int, int]] = []   # (slot, clock, events) of every visit


    def at(self, clock: int, slot: int, events: List[dict]) -> np.ndarray:
        r = visit(self.path, slot, clock, events, self.min_ttl)
        assert len(r) <= self.world.max_events
        self.visits.setdefault(clock, []).append(r)
        self.last[slot] = int(r["ts"][-1])
        self.log.append((slot, clock, len(r)))
        return r

    def flush(self) -> None:
        """One step per clock, or several where the visits exceed the store's dedup capacity: a
        visit is never split (its multiplicity selects the path)."""
        for clock in sorted(self.visits):
            groups: List[List[np.ndarray]] = [[]]
            for r in self.visits[clock]:
                if sum(len(x) for x in groups[-1]) + len(r) > self.world.max_events:
                    groups.append([])
                groups[-1].append(r)
            for g in groups:
                part = interleave(g)
                if self.path in SCORE_PATHS:
                    self.steps.append(Step("score", part, clock))
                else:
                    self.steps.append(Step("probe", probe_rows(range(self.n_acc), clock), clock))
                    self.steps.append(Step("ingest", part, clock))
        self.visits = {}

    def prior(self, rows: np.ndarray) -> None:
        """State from before the edge: always plain ingestion."""
        self.flush()
        self.steps.append(Step("ingest", rows, setup=True))

    def finish(self, *clocks: int) -> List[Step]:
        self.flush()
        for c in clocks:
            self.steps.append(Step("probe", probe_rows([-1] + list(range(self.n_acc)), c), c))
        return self.steps


def _bucket(steps: List[Step]) -> int:
    n = max([len(s.rows) for s in steps if s.kind != "ingest"] + [1])
    return 64 if n <= 64 else 256 if n <= 256 else 1024


def _case(name, path, edge, world, n_acc, steps, focus=0, builder: Optional[Builder] = None) -> Case:
    return Case(f"{edge}_{name}_{path}" if name else f"{edge}_{path}", world, default_batch(n_acc), steps,
                bucket=_bucket(steps), path=path, edge=edge, focus=focus, always_update=path in ("seg_list", "seg_hot"),
                visits=tuple(builder.log) if builder else ())


def ttl_case(path: str, ttlset: str) -> Case:
    """For session, sum, hll_dev, hll_ip and last_tx an account whose next visit comes at exp - 1
    (slot 2 i) and one at exp (slot 2 i + 1). The HLL accounts get a visit without the hash in
    between, which must leave the expiry alone; the visit at exactly the old expiry resets the file."""
    w = World(ttl=ttlset, sum_mode="compat" if ttlset == "small" else "sliding")
    ttls, k = w.ttls(), PATH_K[path]
    b = Builder(path, w, 10)
    t0 = NOW - 8 * 86400
    for s in range(10):
        b.at(t0, s, [event()] * k)
    last0 = dict(b.last)
    for i, kind in enumerate(("session", "sum", "hll_dev", "hll_ip", "last_tx")):
        for side in (0, 1):
            s = 2 * i + side
            exp = last0[s] + ttls[kind]
            if kind.startswith("hll"):
                b.at(last0[s] + 100, s, [event(dev=0, ip=IP1) if kind == "hll_dev" else event(dev=DEV1, ip=0)] * k)
            b.at(exp - 1 + side, s, [event(dev=DEV1, ip=IP1)] * k)
    end = max(b.last.values())
    return _case(ttlset, path, "ttl", w, 10, b.finish(end + 1, end + ttls["session"]), builder=b)


def switch_case(path: str, ttlset: str) -> Case:
    """Segments of 2, 20 and 64 events whose span is min_ttl - 1 (parallel) or min_ttl (serial): the
    last event finds the shortest key expired. ing_scan: the first 64-event chunk of 70 events, and
    the remainder chunk of 2 and of 20 events behind 64 events one second apart, on both sides."""
    w = World(ttl=ttlset, sum_mode="compat")
    m = w.min_ttl()
    span = m - 1 if path == "ing_list_parallel" else m
    items, s = [], 0
    # (events, events of the chunk at the switch, its span); ing_scan: that chunk is the first or the remainder
    sizes = ([(k, k, span) for k in (2, 20, 64)] if path != "ing_scan" else
             [(70, 64, m - 1), (70, 64, m)] + [(64 + r, r, sp) for r in (2, 20) for sp in (m - 1, m)])
    for k, body, sp in sizes:
        if k > 64 and body < 64:   # a first chunk one second apart, then the remainder chunk over the span
            ts = [NOW + j for j in range(64)] + [NOW + 64 + (j * sp) // (body - 1) for j in range(body)]
        else:
            ts = [NOW + (j * sp) // (body - 1) for j in range(body)] + [NOW + sp + 1 + j for j in range(k - body)]
        items.append(rows_of([(s, t, 100 + j, j % 6, hash_for(30 + j % 5, 3 + j % 4, j), hash_for(90 + j % 3, 5, j))
                              for j, t in enumerate(ts)]))
        s += 1
    steps = [Step("ingest", rows_of([(a, NOW - 10, 77, 0, DEV0, IP0) for a in range(s)]), setup=True),
             Step("ingest", interleave(items))]
    end = NOW + m + 150
    steps += [Step("probe", probe_rows(range(s), c), c) for c in (end, end + m)]
    return _case(ttlset, path, "switch", w, s, steps, focus=0)


def ring_wrap_case(path: str) -> Case:
    """ring_size 64: a visit that starts two entries (one for the single-event paths) before the
    end of the ring, then another."""
    w, k = World(ring=64), PATH_K[path]
    b = Builder(path, w, 2)
    n0 = 63 if k == 1 else 62
    b.prior(rows_of([(0, NOW - 4000 + j, 9 + j, 2, DEV0, IP0) for j in range(n0)]))
    for q in range(3):
        b.at(NOW + 7 * q, 0, [event(amount=1000 * (q + 1) + j) for j in range(k)])
        b.flush()
    return _case("", path, "ring_wrap", w, 2, b.finish(NOW + 30), builder=b)


def ring_overrun_case(path: str) -> Case:
    """ring_size 64 and 64 (DEDUP_LIST: still a list segment), 65, 129 and 200 events of one account in one
    batch: entries a later event of the batch overwrites are skipped; the ring equals the sequential result."""
    w = World(ring=64)
    b = Builder(path, w, 4)
    b.prior(rows_of([(s, NOW - 100 + j, 5 + j, 2, DEV0, IP0) for s in range(4) for j in range(10)]))
    for s, k in enumerate((64, 65, 129, 200)):
        b.at(NOW, s, [event(amount=10 * s + j, tx_type=j % 6) for j in range(k)])
    return _case("", path, "ring_overrun", w, 4, b.finish(NOW + 5), focus=3, builder=b)


def hot_tail(ev_ring: int) -> int:
    return min(-(-max(ev_ring, 1) // 64) * 64, HOT_TAIL_MAX)


def ev_ring_case(path: str, ev_ring: int) -> Case:
    """DEDUP_LIST + 1, T, T + 1 and 300 events of one account in one batch (T: the hot tail of the
    event ring), twice: ev_head wraps, ev_count saturates, the rows are the last event_ring events'."""
    w = World(ev_ring=ev_ring)
    T = hot_tail(ev_ring)
    counts = sorted({DEDUP_LIST + 1, T, T + 1, 300} | ({ev_ring + 1} if ev_ring > DEDUP_LIST else set()))
    b = Builder(path, w, len(counts))
    for q in range(2):
        for s, k in enumerate(counts):
            b.at(NOW + 40 * q, s, [event(amount=7 * j + s, tx_type=j % 7,
                                         dev=hash_for((3 * j + q) % 256, 1 + j % 9, j), ip=hash_for(j % 50, 2 + q, j))
                                   for j in range(k)])
        b.flush()
    return _case(f"e{ev_ring}", path, "ev_ring", w, len(counts), b.finish(NOW + 100), focus=len(counts) - 1,
                 builder=b)


def ev_head_case(path: str) -> Case:
    """event_ring 12: the head wraps and the count saturates on every path (three visits). The
    multi-event paths bring more events than the ring holds in one segment (a K1 leader 14): only
    the last 12 rows stay, and lanes of one wave must not write one ring position twice."""
    w, k = World(ev_ring=12), max(PATH_K[path], 14 if PATH_K[path] > 1 else 1)
    b = Builder(path, w, 2)
    b.prior(rows_of([(0, NOW - 900 + j, 3 * j, j % 6, DEV0, IP0) for j in range(10)]))
    for q in range(3):
        b.at(NOW + 11 * q, 0, [event(amount=500 * q + j, tx_type=(q + j) % 6) for j in range(k)])
        b.flush()
    return _case("", path, "ev_head", w, 2, b.finish(NOW + 50), builder=b)


def _hll_scenarios() -> Dict[str, List[dict]]:
    d = lambda reg, rank, salt=0: hash_for(reg, rank, salt)  # noqa: E731
    return {
        "repeat": [event(dev=d(7, 4, 1), ip=d(7, 4, 1))] * 3,
        "high_first": [event(dev=d(8, 9, 1), ip=d(8, 2, 5)), event(dev=d(8, 2, 2), ip=d(8, 9, 6)),
                       event(dev=d(8, 9, 3), ip=d(8, 9, 7))],
        "low_first": [event(dev=d(9, 2, 1), ip=0), event(dev=d(9, 9, 2), ip=d(9, 1)), event(dev=d(9, 5, 3), ip=d(9, 1))],
        "one_word": [event(dev=d(4, 3), ip=d(5, 3)), event(dev=d(5, 6), ip=d(6, 2)), event(dev=d(7, 1), ip=d(4, 8))],
        "below": [event(dev=d(12, 5, 1), ip=d(12, 20, 2)), event(dev=d(12, 20, 3), ip=d(12, 19, 4))],  # after rank 20
        "many_regs": [event(dev=d(100 + j, 1 + j % 5, j), ip=d(200 - 2 * j, 3, j)) for j in range(12)],
        "rank57": [event(dev=d(77, 57), ip=d(78, 56)), event(dev=d(77, 56, 0), ip=d(78, 57))],
        "hash0_first": [event(dev=0, ip=0), event(dev=d(13, 2), ip=0), event(dev=0, ip=d(13, 2))],
        "reset_rise": [event(dev=d(14, 3), ip=d(14, 3)), event(dev=d(15, 1), ip=0)],  # at the old expiry
    }


HLL_SCENARIOS = tuple(_hll_scenarios())


def hll_case(path: str, tail: bool = True) -> Case:
    """One account per scenario. Single-event paths: event j of every scenario is step j. The
    paths of more than DEDUP_LIST events get the scenario in front of (seg_hot: the bulk, whose
    registers are a per-register max) or behind (the exact tail; ing_scan: the third chunk) plain
    events, 150 in all: with the hot tail of 128 events the bulk holds 22, more than any scenario.
    ``chosen`` records where the scenario's events sit (tests/test_k1_edges.py checks it)."""
    w = World()
    sc = _hll_scenarios()
    names = list(sc)
    b = Builder(path, w, len(names))
    t0 = NOW - w.ttls()["hll_dev"]          # reset_rise: the prior event's expiry is NOW, its visit starts with a
    prior = [(s, t0 + (0 if n == "reset_rise" else 50), 1, 0, hash_for(12, 20, 9), hash_for(12, 20, 9))
             for s, n in enumerate(names)]  # reset; the others' registers (rank 20 on register 12) are alive at NOW
    b.prior(rows_of(prior))
    k = PATH_K[path]
    chosen = []
    if k == 1:
        for j in range(max(len(v) for v in sc.values())):
            for s, n in enumerate(names):
                if j < len(sc[n]):
                    b.at(NOW + 3 * j, s, [sc[n][j]])
            b.flush()
    else:
        for s, n in enumerate(names):
            ev = sc[n]
            if k > DEDUP_LIST:
                ev = padded(path, ev, tail=tail, k=150)
                chosen.append((s, 150 - len(sc[n]), 149, 150) if tail else (s, 0, len(sc[n]) - 1, 150))
            elif path == "seg_list" and n in ("many_regs", "repeat"):
                ev = padded(path, ev, tail=True, k=64 if n == "many_regs" else 17)
            elif len(ev) < 2:
                ev = padded(path, ev, k=2)
            b.at(NOW, s, ev)
    name = "" if k <= DEDUP_LIST else ("tail" if tail else "bulk")
    c = _case(name, path, "hll", w, len(names), b.finish(NOW + 60), focus=names.index("many_regs"), builder=b)
    c.chosen = tuple(chosen)
    return c


def hll_switch_n(rank: int = 30) -> int:
    """The smallest number of distinct registers (all of ``rank``) at which hll_estimate leaves the
    linear-counting table for the harmonic mean: alpha m^2 / z > 2.5 m (golden.hll.count)."""
    for n in range(1, GH.M + 1):
        z = (GH.M - n) + n * 2.0 ** -rank
        if GH.ALPHA * GH.M * GH.M / z > 2.5 * GH.M:
            return n
    raise AssertionError


def hll_fill_case(path: str) -> Case:
    """One account on each side of the estimator's switch from linear counting to the harmonic
    mean, and one whose 256 hashes fill every register (no zero register left)."""
    n_sw = hll_switch_n()
    w = World()
    b = Builder(path, w, 3)
    for s, n in enumerate((n_sw - 1, n_sw, 256)):
        # (the full files get small ranks: 256 registers of rank 30 would be an estimate beyond int32)
        b.at(NOW, s, [event(amount=j, dev=hash_for(j, 30 if s < 2 else 1 + j % 7, j),
                            ip=hash_for(255 - j, 30 if s < 2 else 1 + j % 11, j)) for j in range(n)])
    return _case("", path, "hll_fill", w, 3, b.finish(NOW + 9), focus=2, builder=b)


FIELD_EVENTS = ([event(amount=a, tx_type=0) for a in (0, -5, 99999, 100000)] +
                [event(amount=321, tx_type=t) for t in (0, 1, 2, 3, 4, 5, 7)])


def fields_case(path: str) -> Case:
    """Event rows: amount 0, negative, 99999 / 100000; tx_type 0..5 and 7; dt 0 (two events at one
    clock) and, on the ingestion paths, a predecessor later than the event (dt -> 0)."""
    w, k = World(ev_ring=64), PATH_K[path]
    b = Builder(path, w, 2)
    b.prior(rows_of([(0, NOW - 5, 1, 0, DEV0, IP0), (1, NOW + 500, 1, 0, DEV0, IP0)]))  # account 1: prev > ts
    if k == 1:
        for j, e in enumerate(FIELD_EVENTS):
            b.at(NOW + (j // 2), 0, [e])      # pairs at one clock: dt 0
            b.at(NOW + (j // 2), 1, [e])
            b.flush()
    else:
        for s in (0, 1):
            b.at(NOW, s, padded(path, FIELD_EVENTS, tail=True))
    return _case("", path, "fields", w, 2, b.finish(NOW + 20), builder=b)


def row_order_case(path: str, ttlset: str) -> Case:
    """An ingested segment whose row order is not time order (rows are applied in row order)."""
    w = World(ttl=ttlset, sum_mode="compat", ev_ring=64)
    m, k = w.min_ttl(), PATH_K[path]
    span = m // 2 if path != "ing_list_serial" else 3 * m
    off = [(j * 7919) % (span + 1) for j in range(k)]
    off[0], off[1] = span, 0
    rows = rows_of([(0, NOW + o, 50 + j, j % 6, hash_for(j % 7, 2 + j % 3, j), hash_for(9 + j % 4, 4, j))
                    for j, o in enumerate(off)])
    steps = [Step("ingest", rows_of([(0, NOW - 20, 5, 0, DEV0, IP0)]), setup=True), Step("ingest", rows)]
    steps += [Step("probe", probe_rows([0, 1], c), c) for c in (NOW + span + 1, NOW + span + m)]
    return _case(ttlset, path, "row_order", w, 2, steps)


def collision_case(path: str) -> Case:
    """Two accounts of one scoring batch with the same home slot in the dedup region: both with a
    single event (k1_single), or the second one a K1 leader with three."""
    w = World(max_events=256)
    s1, s2 = colliding_slots(w.max_events)
    b = Builder(path, w, 64)
    b.prior(rows_of([(s, NOW - 100, 5, 0, DEV0, IP0) for s in (s1, s2)]))
    for q in range(2):
        b.at(NOW + q, s1, [event(amount=11 + q)])
        b.at(NOW + q, s2, [event(amount=500 + j + q, dev=DEV1) for j in range(PATH_K[path])])
        b.at(NOW + q, 3, [event(amount=9)])
        b.flush()
    c = _case("", path, "collision", w, 64, b.finish(NOW + 10), focus=s2, builder=b)
    return c


def tables_leader_case() -> Case:
    """A K1 leader probes the tables for its account's other rows (its own probe loop)."""
    w = World(tables="edges")
    b = Builder("k1_leader", w, 3)
    ev = [event(amount=100001 + i, tx_type=i % 3, dev=d, fp=f, ip=p) for i, (d, f, p) in enumerate(TABLE_KEYS[:16])]
    b.at(NOW, 0, ev)
    b.at(NOW, 1, ev[8:] + ev[:2])
    return _case("", "k1_leader", "tables", w, 3, b.finish(NOW + 1), builder=b)


# the path x edge matrix: which paths can meet which edge
MATRIX = {
    "ttl": PATHS, "ring_wrap": PATHS, "ev_head": PATHS, "hll": PATHS, "fields": PATHS,
    "switch": ("ing_list_parallel", "ing_list_serial", "ing_scan"),
    "row_order": ("ing_list_parallel", "ing_list_serial", "ing_scan"),
    "ring_overrun": ("seg_hot", "ing_scan"),
    "ev_ring": ("seg_hot", "ing_scan"),
    "hll_fill": ("seg_hot", "ing_scan"),
    "collision": ("k1_single", "k1_leader"),
    "tables": ("k1_leader",),
}
LEFT_OUT: Dict[Tuple[str, str], str] = {}   # (path, edge) -> reason; nothing is left out
READ_LEFT_OUT = {   # read-path edges of the issue that no case holds, with the reason
    "sparse ring beyond position 3": "ingestion and scoring fill a tx ring from its head, so an entry at position "
                                     "63, 64, 255, 256 or R - 1 always has non-empty entries before it; those "
                                     "positions are probed in full and wrapped rings whose other entries lie outside "
                                     "the hour, and only positions 0-3 in rings that are empty elsewhere",
}
EV_RINGS = (12, 64, 100, 192, 256)


def write_cases() -> List[Case]:
    out: List[Case] = []
    for p in PATHS:
        out += [ttl_case(p, "default"), ttl_case(p, "small"), ring_wrap_case(p), ev_head_case(p), fields_case(p)]
        out += [hll_case(p)] + ([hll_case(p, tail=False)] if PATH_K[p] > DEDUP_LIST else [])
    for p in MATRIX["switch"]:
        out += [switch_case(p, "default"), switch_case(p, "small")]
        out += [row_order_case(p, "default"), row_order_case(p, "small")]
    for p in MATRIX["ring_overrun"]:
        out += [ring_overrun_case(p), hll_fill_case(p)] + [ev_ring_case(p, e) for e in EV_RINGS]
    out += [collision_case(p) for p in MATRIX["collision"]] + [tables_leader_case()]
    return out


_CASES: Optional[List[Case]] = None


def all_cases() -> List[Case]:
    global _CASES
    if _CASES is None:
        _CASES = read_cases() + write_cases()
        assert len({c.name for c in _CASES}) == len(_CASES)
    return _CASES


# ------------------------------------------------------------------------------------ paths
def focus_shape(case: Case) -> Tuple[str, int, int, int]:
    """(via, count, span, batch_max) of the focus account's largest visit: how the events arrive,
    how many in one step, the span of their ts and the largest multiplicity of that step."""
    via = "score" if case.path in SCORE_PATHS else "ingest"
    best = (via, 0, 0, 0)
    for st in case.steps:
        if st.kind != via or st.setup:
            continue
        mine = st.rows[st.rows["slot"] == case.focus]
        if len(mine) > best[1]:
            ts = mine["ts"]
            slots = st.rows["slot"][st.rows["slot"] >= 0]
            best = (via, len(mine), int(ts.max() - ts.min()) if via == "ingest" else 0,
                    int(np.bincount(slots).max()))
    return best


def expected_path(case: Case) -> str:
    """Who applies the focus account's events, from the project's constants (K1_SEG_MAX, DEDUP_LIST,
    the minimum of the four TTLs) and the case's steps."""
    via, c, span, batch_max = focus_shape(case)
    if via == "score":
        if c == 1:
            return "k1_single"
        if c > DEDUP_LIST:
            return "seg_hot"
        if c <= k1_seg_max() and batch_max <= k1_seg_max() and not case.always_update:
            return "k1_leader"
        return "seg_list"
    if c == 1:
        return "ing_single"
    if c > DEDUP_LIST:
        return "ing_scan"
    return "ing_list_serial" if span >= case.world.min_ttl() else "ing_list_parallel"
