"""ScoreBatch bytes through the native serving core on the GPU pipeline with a 64-row device
batch: requests of 65 and 130 transactions span two and three steps, so their later segments
are serialised from a slot's pinned result / feature buffers at a non-zero device position
(and a first segment may sit behind another request's rows). The answers must be the CPU
engine's for the same stream, byte for byte once response_time_ms is cleared."""
import numpy as np
import pytest

from igaming_platform_amd.config import Config
from igaming_platform_amd.layouts import ACCTBATCH

from .test_ingress_path import strip_response_ms

pytestmark = pytest.mark.gpu
NOW = 1_760_000_000


def _txs(n, rng, n_acc=40):
    types = ["deposit", "withdraw", "bet", "win", "bonus"]
    return [dict(account_id=f"acc-{int(a)}", amount=int(rng.choice([500, 5000, 150000, 3_000_000_000])),
                 transaction_type=types[int(rng.integers(0, 5))], device_id=f"dev-{int(a)}-{int(rng.integers(0, 5))}",
                 ip_address=f"10.1.{int(a)}.{int(rng.integers(0, 7))}", fingerprint=f"fp-{int(a)}")
            for a in rng.integers(0, n_acc, n)]


def test_segments_at_nonzero_device_positions_equal_cpu_engine():
    from igaming_platform_amd.engine.risk_engine import RiskEngine
    from igaming_platform_amd.proto import risk_v1 as P
    cfg = Config()
    cfg.gpu.buckets = [64]
    cfg.gpu.max_batch = 64
    g = RiskEngine(cfg, backend="gpu", capacity=4096)
    c = RiskEngine(cfg, backend="cpu", capacity=4096)
    assert g.core is not None and c.core is not None
    rng = np.random.default_rng(0)
    ids = [f"acc-{i}" for i in range(40)]
    rows = np.zeros(40, ACCTBATCH)
    rows["present"] = 1
    rows["total_deposits"] = rng.integers(0, 10**6, 40)
    rows["total_withdrawals"] = rng.integers(0, 10**6, 40)
    rows["deposit_count"] = rng.integers(0, 5, 40)
    rows["bonus_claim_count"] = rng.integers(0, 6, 40)
    rows["account_created_at"] = NOW - rng.integers(0, 30, 40) * 86400
    for e in (g, c):
        e.load_batch_features(ids, rows)
        e.add_to_blacklist("device", "dev-3-1", "x", "t")
        e.set_ip_intel("10.1.5.2", vpn=True)
    steps0 = g.core.stats()["steps"]
    for k, n in enumerate((65, 130, 130, 65)):
        data = P.ScoreBatchRequest(transactions=[P.ScoreTransactionRequest(**t) for t in _txs(n, rng)]).SerializeToString()
        got = g.score_batch_bytes(data, now=NOW + 40 * k)
        want = c.score_batch_bytes(data, now=NOW + 40 * k)
        a, b = P.ScoreBatchResponse.FromString(got), P.ScoreBatchResponse.FromString(want)
        assert len(a.results) == len(b.results) == n
        for i, (x, y) in enumerate(zip(a.results, b.results)):
            x.response_time_ms = y.response_time_ms = 0
            assert x == y, (k, i)
        assert strip_response_ms(got) == strip_response_ms(want)
    st = g.core.stats()
    assert st["max_step_rows"] <= 64 and st["steps"] - steps0 >= 2 + 3 + 3 + 2
    assert st["copy_ns"] == 0   # serialised from the slots, nothing staged
    # the last step's D2H feature images: the device encoded them (records.h FV_IMG_ENCODED)
    sc = g.backends[0].scorer
    img = np.stack([h.numpy().view(np.uint8).reshape(-1, 128) for h in sc.host_feat])
    assert int(((img[:, :, 127] & 0x80) != 0).sum()) > 0
