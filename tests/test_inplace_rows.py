"""ScoreBatch rows read in place: the serving core resolves a request's rows into a pinned buffer
of its pool and a step names its segments in the slot's segment table (device_ops.h) instead of
packing them into the slot's request buffer. ServeCore on CpuDevice, whose submit gathers the
segments as the GPU's dedup insert reads them.

The answers must not depend on the mode, a step that cannot run in place (more than IGP_ROW_SEGS
segments, a unary call in it) is packed as before, and a buffer stays out of the pool for as long
as a step may still read it - a late step reading a later request's rows would apply them to the
feature store.

What a row is answered depends on which earlier rows of its account sat in EARLIER steps, so a
stream compares byte-equal between two stacks only where its cut into steps is the same on both:
* requests sent one at a time are cut at the step capacity, always in the same places - these
  carry the accounts that repeat within a step and from step to step;
* requests sent from four threads at once are cut wherever the other threads' rows fall - their
  accounts appear once per request and repeat only from one request of a thread to its next."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from igaming_platform_amd.config import Config
from igaming_platform_amd.native import native
from tests.test_ingress_path import NOW, batch, random_txs, strip_response_ms, tx, uuid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 37, 64, 100, 129]
ROW_SEGS = 16


class Stack:
    """Account index + CPU scorer + CpuDevice + ServeCore, world 1, step capacity 64."""

    def __init__(self, inplace, cap=64, depth=2, max_wait_us=200, accounts=8192):
        from igaming_platform_amd.engine.backends import NativeCpuBackend
        N = native()
        self.backend = NativeCpuBackend(Config(), accounts)
        self.index = N.AccountIndex(accounts)
        self.device = self.backend.native_device(depth=depth, cap=cap, inplace=inplace)
        self.core = N.ServeCore([self.index], self.device, 0, None, max_wait_us=max_wait_us, features=True)

    def ask(self, data):
        return strip_response_ms(self.core.score_batch(data, NOW))

    def close(self):
        self.core.stop()


def _spin(cond, what):
    """Poll for a state another thread is about to reach (no fixed sleep; 20 s is a failure)."""
    t_end = time.monotonic() + 20
    while not cond():
        assert time.monotonic() < t_end, what
        time.sleep(0.0005)


def _serial_stream():
    """One sender: every size, over 40 accounts, so that accounts repeat within a step (100 and 129
    rows over 40 accounts), across the steps of one request and from request to request."""
    rng = np.random.default_rng(11)
    ids = [uuid(rng) for _ in range(40)]
    return [batch(random_txs(rng, n, ids[k:] + ids[:k])) for k, n in enumerate(SIZES + SIZES[::-1])]


def _thread_streams():
    """Four senders at once: each request's accounts appear once in it and again in the thread's
    later requests (a thread's request is answered before it sends the next)."""
    out = []
    for t in range(4):
        rng = np.random.default_rng(200 + t)
        ids = [f"t{t}-{i}" if i % 2 else uuid(rng) for i in range(129)]
        order = SIZES[t:] + SIZES[:t]
        out.append([batch(random_txs(rng, n, ids[:n])) for n in order + order])
    return out


def _run_streams(stack):
    got = {"serial": [stack.ask(d) for d in _serial_stream()]}
    streams, errs = _thread_streams(), []
    start = threading.Barrier(len(streams))

    def run(t):
        try:
            start.wait()
            got[t] = [stack.ask(d) for d in streams[t]]
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=run, args=(t,)) for t in range(len(streams))]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not errs, errs
    return got


def test_answers_are_byte_equal_in_place_and_packed():
    on, off = Stack(True), Stack(False)
    try:
        a, b = _run_streams(on), _run_streams(off)
        assert a.keys() == b.keys()
        for k in a:
            assert a[k] == b[k], k
        s_on, s_off = on.core.stats(), off.core.stats()
        rows = 2 * sum(SIZES) * 5
        assert s_on["rows"] == s_off["rows"] == rows and s_on["max_step_rows"] <= 64
        # 100 and 129 rows at capacity 64: requests are split in the middle, and every such step ran in place
        assert s_on["inplace_steps"] > 0 and s_on["packed_steps"] == 0
        assert s_on["inplace_steps"] == s_on["steps"] >= 2 * (1 + 1 + 1 + 2 + 3)
        assert on.device.gathered_steps == s_on["inplace_steps"]
        assert s_off["inplace_steps"] == 0 and s_off["packed_steps"] == s_off["steps"] and off.device.gathered_steps == 0
        assert s_off["rowbufs"] == 0 and 1 <= s_on["rowbufs"] == s_on["rowbufs_free"]
    finally:
        on.close()
        off.close()
    assert on.core.stats()["rowbufs"] == 0


def _held_step(stack, salt):
    """Make one step late and hold it: the pipeline then has a step in flight, so the stepper forms
    the next step only from a full capacity of queued rows (max_wait_us is out of reach), and the
    completion thread answers nothing until debug_release_steps()."""
    rng = np.random.default_rng(5)
    stack.device.debug_hold_steps(1)
    with pytest.raises(RuntimeError, match="exceeded its deadline"):
        stack.core.score_batch(batch(random_txs(rng, 5, [f"{salt}-{i}" for i in range(5)])), NOW)
    _spin(lambda: stack.device.debug_held_steps() == 1, "the late step is not held")


def _fresh(rng, n, salt):
    """A request over n accounts nothing else uses: answered the same however it is cut."""
    return batch(random_txs(rng, n, [f"{salt}-{i}" for i in range(n)]))


def test_step_with_more_segments_than_the_table_is_packed():
    rng = np.random.default_rng(21)
    small = [_fresh(rng, 1 + k % 3, f"s{k}") for k in range(20)]
    filler = _fresh(rng, 64, "fill")
    on, off = Stack(True, max_wait_us=60_000_000), Stack(False)
    try:
        want = [off.ask(d) for d in small] + [off.ask(filler)]
        _held_step(on, "held")
        on.core.stats(True)
        got, errs = [None] * 21, []

        def run(k, d):
            try:
                got[k] = on.ask(d)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=run, args=(k, d)) for k, d in enumerate(small)]
        for x in th:
            x.start()
        _spin(lambda: on.core.pending_items() == 20, "20 small requests queued")
        tf = threading.Thread(target=run, args=(20, filler))   # fills the step: 20 + 1 segments in it
        tf.start()
        _spin(lambda: on.core.stats()["steps"] >= 1, "the full step was issued")
        st = on.core.stats()
        assert st["packed_steps"] == 1 and st["inplace_steps"] == 0 and st["max_step_rows"] == 64
        assert 20 + 1 > ROW_SEGS
        on.device.debug_release_steps()
        for x in th + [tf]:
            x.join()
        assert not errs, errs
        assert got == want
        st = on.core.stats()
        assert st["packed_steps"] == 1 and st["inplace_steps"] >= 1   # the filler's other rows: one segment, in place
    finally:
        on.device.debug_release_steps()
        on.close()
        off.close()


def test_unary_call_in_a_step_with_a_batch_item_is_packed():
    rng = np.random.default_rng(22)
    one = tx("unary-acct", 700, "deposit")
    req = _fresh(rng, 64, "mixed")
    on, off = Stack(True, max_wait_us=60_000_000), Stack(False)
    try:
        off.core.submit_tx(one, 7, NOW)
        _spin(lambda: off.core.pending_items() == 0, "unary call taken")
        (tag_w, bytes_w, err_w), = off.core.poll(timeout_us=20_000_000)
        want = off.ask(req)
        _held_step(on, "held")
        on.core.stats(True)
        on.core.submit_tx(one, 7, NOW)
        out = {}
        t = threading.Thread(target=lambda: out.setdefault("b", on.ask(req)))
        t.start()
        _spin(lambda: on.core.stats()["steps"] >= 1, "the mixed step was issued")
        st = on.core.stats()
        assert st["packed_steps"] == 1 and st["inplace_steps"] == 0 and st["unary"] == 1 and st["max_step_rows"] == 64
        on.device.debug_release_steps()
        t.join()
        (tag_g, bytes_g, err_g), = on.core.poll(timeout_us=20_000_000)
        assert (tag_g, err_g) == (tag_w, err_w) == (7, None)
        from igaming_platform_amd.proto import risk_v1 as P
        a, b = P.ScoreTransactionResponse.FromString(bytes_g), P.ScoreTransactionResponse.FromString(bytes_w)
        a.response_time_ms = b.response_time_ms = 0
        assert a == b
        assert out["b"] == want
    finally:
        on.device.debug_release_steps()
        on.close()
        off.close()


def test_buffer_of_a_failed_item_stays_out_of_the_pool_while_its_step_is_held():
    rng = np.random.default_rng(23)
    later, after = _fresh(rng, 37, "later"), [_fresh(rng, n, f"after{n}") for n in (1, 100, 129)]
    on, off = Stack(True), Stack(False)
    try:
        want_later, want_after = off.ask(later), [off.ask(d) for d in after]
        # the failed item returned its error (inside _held_step); the step it rode in is held
        _held_step(on, "held")
        st = on.core.stats()
        assert st["rowbufs"] == 1 and st["rowbufs_free"] == 0, "the held step's buffer went back to the pool"
        out = {}
        t = threading.Thread(target=lambda: out.setdefault("r", on.ask(later)))
        t.start()
        # the later request did not get that buffer: the pool had none, a second one was allocated
        _spin(lambda: on.core.stats()["rowbufs"] == 2, "the later request took no new buffer")
        assert on.core.stats()["rowbufs_free"] == 0 and "r" not in out
        on.device.debug_release_steps()
        t.join()
        assert out["r"] == want_later
        _spin(lambda: on.core.stats()["rowbufs_free"] == 2, "both buffers back once the step was released")
        assert [on.ask(d) for d in after] == want_after
        # a step that fails in submit: the item fails, nothing is held, nothing leaks
        on.device.debug_fail_steps(1, 0)
        with pytest.raises(RuntimeError, match="injected step failure"):
            on.core.score_batch(_fresh(rng, 37, "failed"), NOW)
        _spin(lambda: on.core.stats()["rowbufs_free"] == on.core.stats()["rowbufs"], "a buffer leaked")
        again = _fresh(rng, 65, "again")
        assert on.ask(again) == off.ask(again)
        assert on.core.stats()["rowbufs"] >= 1
    finally:
        on.device.debug_release_steps()
        on.close()
        off.close()
    st = on.core.stats()
    assert st["rowbufs"] == 0 and st["rowbufs_free"] == 0   # stop() freed every buffer


@pytest.mark.timeout(600)
def test_inplace_rows_check_program_under_asan_ubsan(tmp_path):
    """tools/inplace_rows_check.cpp: the three cases above driven from several threads by a
    stand-alone program (ServeCore + CpuDevice, no Python), built with ASan + UBSan."""
    import glob
    srcs = [s for s in sorted(glob.glob(os.path.join(ROOT, "csrc", "runtime", "*.cpp")))
            if os.path.basename(s) not in ("bindings.cpp",)]
    exe = str(tmp_path / "inplace_rows_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "csrc", "include"),
           "-I" + os.path.join(ROOT, "csrc", "runtime"), os.path.join(ROOT, "tools", "inplace_rows_check.cpp"),
           *srcs, "-o", exe, "-lpthread", "-lrt"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=540)
    assert p.returncode == 0, p.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    out = p.stdout + p.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert p.returncode == 0, out[-4000:]
    assert "inplace_rows_check: ok" in out
