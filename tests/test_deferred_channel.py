"""The deferred status channel of caspr_amd/ops.py on the CPU: ordering, backlog, buffer pool, the six reporters and the conv guard's
coalescing, with plain CPU tensors for the pinned buffers and device words and a fake event for the copy's arrival."""
import math
import warnings

import pytest
import torch

from caspr_amd import ops
from caspr_amd.lib import CasprHipError

KEY = (0, 7)


class FakeEvent:
    def __init__(self, arrived):
        self.arrived, self.synced = arrived, 0

    def query(self):
        return self.arrived

    def synchronize(self):
        self.synced += 1
        self.arrived = True


class Device:
    """What the fakes saw: the buffers allocated, the events recorded (arrived at once or not: `arrives`), the words zeroed."""

    def __init__(self):
        self.arrives, self.allocated, self.events, self.zeroed = True, [], [], []


@pytest.fixture()
def device(monkeypatch):
    d = Device()

    def pinned(n, dtype):
        d.allocated.append(torch.full((n,), -1, dtype=dtype))      # no fill value is promised: the copy must overwrite all of it
        return d.allocated[-1]

    def copy_behind(host, src, stream=None):
        host.copy_(src)
        d.events.append(FakeEvent(d.arrives))
        return d.events[-1]

    monkeypatch.setattr(ops, "_pinned", pinned)
    monkeypatch.setattr(ops, "_copy_behind", copy_behind)
    monkeypatch.setattr(ops, "_zero_word", lambda word, stream: (word.zero_(), d.zeroed.append(word)))
    return d


@pytest.fixture()
def seen():
    """A channel whose reporter only notes what it was handed."""
    got = []
    chan = ops._Deferred(got.append)
    chan.got = got
    return chan


@pytest.fixture()
def channels(device):
    """The module's six channels, empty before and after."""
    chans = (ops._team, ops._latent_dp5, ops._cnf_h3, ops._conv_h3, ops._steps, ops._guard)

    def clear():
        for c in chans:
            c.rings.clear()
            c.pool.clear()
        for c in (ops._cnf_h3, ops._conv_h3):
            c.words.clear()
        ops._conv_h3.stale.clear()
        ops.reset_guard()
    clear()
    yield chans
    clear()


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def test_records_drain_oldest_first(device, seen):
    for n in (1, 2, 3):
        seen.post(KEY, i32(n), "m%d" % n)
    seen.post((0, 8), i32(9))
    seen.poll(KEY)
    assert seen.got == [[([1], "m1"), ([2], "m2"), ([3], "m3")]]
    assert seen.rings[KEY] == [] and len(seen.rings[(0, 8)]) == 1, "a poll drains its own key only"
    seen.poll_all()
    assert seen.got[1:] == [[([9], None)]]
    seen.poll_all(wait=True)
    assert len(seen.got) == 2, "nothing outstanding: the reporter is not called"


def test_no_wait_stops_at_the_first_record_that_has_not_arrived(device, seen):
    seen.post(KEY, i32(1))
    device.arrives = False
    seen.post(KEY, i32(2))
    device.arrives = True
    seen.post(KEY, i32(3))                 # arrived, but behind one that has not
    seen.poll(KEY)
    assert seen.got == [[([1], None)]]
    assert [int(h[0]) for h, _, _ in seen.rings[KEY]] == [2, 3]
    seen.poll(KEY)
    assert len(seen.got) == 1 and len(seen.rings[KEY]) == 2
    assert all(e.synced == 0 for e in device.events), "a poll that does not wait never synchronises"


def test_wait_synchronises_and_drains_everything(device, seen):
    device.arrives = False
    for n in (1, 2, 3):
        seen.post(KEY, i32(n))
    seen.poll_all(wait=True)
    assert seen.got == [[([1], None), ([2], None), ([3], None)]] and seen.rings[KEY] == []
    assert [e.synced for e in device.events] == [1, 1, 1]


def test_with_form_polls_on_entry_and_posts_from_the_body_but_not_under_capture(device, seen, monkeypatch):
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    monkeypatch.setattr(ops._Deferred, "key", staticmethod(lambda dev: KEY))
    with seen.on(None) as status:
        status.post(i32(1), "a")
    assert seen.got == [] and len(seen.rings[KEY]) == 1
    with seen.on(None) as status:
        assert seen.got == [[([1], "a")]], "the earlier launch is reported before the body runs"
        status.post(i32(2), "b")
    capturing[0] = True
    with seen.on(None) as status:
        status.post(i32(3), "c")
    assert len(seen.got) == 1 and [m for _, _, m in seen.rings[KEY]] == ["b"] and len(device.events) == 2
    assert all(e.synced == 0 for e in device.events), "the entry poll does not wait"


def test_a_failed_record_before_a_clean_one_raises_exactly_once(channels):
    ops._team.post(KEY, i32(0, 4))
    ops._team.post(KEY, i32(0, 0))
    with pytest.raises(CasprHipError, match="team barrier gave up"):
        ops._team.poll(KEY)
    ops._team.poll(KEY, wait=True)
    ops.check_deferred_errors()


def test_backlog_bound(device, seen):
    device.arrives = False
    for n in range(64):
        seen.post(KEY, i32(n))
    assert len(seen.rings[KEY]) == 64 and seen.got == [] and all(e.synced == 0 for e in device.events)
    seen.post(KEY, i32(64))                # the 65th: blocks on the oldest, drains what has arrived, then posts
    assert [e.synced for e in device.events[:2]] == [1, 0]
    assert seen.got == [[([0], None)]]
    assert len(seen.rings[KEY]) == 64 and int(seen.rings[KEY][-1][0][0]) == 64


def test_backlog_drain_raises_from_the_posting_call(channels, device):
    device.arrives = False
    ops._team.post(KEY, i32(1))
    for _ in range(63):
        ops._team.post(KEY, i32(0))
    with pytest.raises(CasprHipError):
        ops._team.post(KEY, i32(0))
    assert len(ops._team.rings[KEY]) == 63, "drain first: the call that raised has posted nothing"


def test_pool_reuse_by_size(device, seen):
    for n in (1, 4, 1):
        seen.post(KEY, torch.arange(n, dtype=torch.int32))
        seen.poll(KEY)
    assert [h.numel() for h in device.allocated] == [1, 4], "the third post takes the first buffer back"
    assert seen.got == [[([0], None)], [([0, 1, 2, 3], None)], [([0], None)]]
    seen.post(KEY, torch.zeros(1))         # same size, another dtype: not the int32 buffer
    assert [h.dtype for h in device.allocated] == [torch.int32, torch.int32, torch.float32]


def test_team_reporter(channels):
    ops._team.post(KEY, i32(0, 0, 0, 0))
    ops._team.poll(KEY)
    ops._team.post(KEY, i32(0, 0, 2, 0))
    with pytest.raises(CasprHipError, match="LATENT_TEAM = False"):
        ops._team.poll(KEY)


def test_latent_dopri5_reporter(channels):
    ops._latent_dp5.post(KEY, i32(1, 1, 1), 50)
    ops._latent_dp5.post(KEY, i32(1, 0, 1, 0, 0), 77)      # the first failing record is the one named
    ops._latent_dp5.post(KEY, i32(0, 1), 99)
    with pytest.raises(CasprHipError, match=r"3 of 5 sequences .* max_attempts = 77 attempts") as e:
        ops._latent_dp5.poll(KEY)
    assert "99" not in str(e.value)
    ops._latent_dp5.poll(KEY, wait=True)


@pytest.mark.parametrize("bits,has,lacks", [(1, ['cnf_split="bf16x6"'], ["cnf_dp5_split"]), (2, ['cnf_dp5_split="bf16x6"'], ["cnf_split="]),
                                            (3, ['cnf_split="bf16x6"', 'cnf_dp5_split="bf16x6"'], [])])
def test_cnf_h3_reporter(channels, bits, has, lacks):
    ops._cnf_h3.post(KEY, i32(0))
    for b in (1, 2):
        if bits & b:
            ops._cnf_h3.post(KEY, i32(b))
    with pytest.raises(CasprHipError) as e:
        ops._cnf_h3.poll(KEY)
    assert all(h in str(e.value) for h in has) and not any(l in str(e.value) for l in lacks)
    ops._cnf_h3.post(KEY, i32(0))
    ops._cnf_h3.poll(KEY)


def test_steps_reporter(channels):
    ops._steps.post(KEY, i32(3), (64, 1e-5))
    ops._steps.post(KEY, i32(0), (32, 1e-4))
    ops._steps.post(KEY, i32(5), (128, 1e-3))
    with pytest.raises(ops.CasprAccuracyError) as e:
        ops._steps.poll(KEY)
    assert "3 frame(s) capped at 64 steps (tol 1.0e-05); 5 frame(s) capped at 128 steps (tol 1.0e-03)" in str(e.value)
    assert "capped at 32" not in str(e.value)


def guard_meta(action, name="cnf", tol=1e-3):
    return {"name": name, "tol": tol, "factor": 2.0, "steps": 8, "other_steps": 4, "action": action, "what": "point CNF"}


def guard_post(diff, xmax, meta):
    ops._guard.post(None, torch.tensor([diff, xmax], dtype=torch.float32), meta)


def test_guard_reporter_warns_or_raises(channels):
    guard_post(0.25, 1.0, guard_meta("warn", "latent"))
    with pytest.warns(RuntimeWarning, match="RK4 with 8 steps is not converged") as w:
        ops.check_deferred_errors()
    assert w[0].filename == __file__, "the warning points at the caller of check_deferred_errors"
    last = ops.GUARD_LAST["latent"]
    assert (last["diff"], last["estimate"], last["bound"], last["ok"]) == (0.25, 0.5, 1e-3 * 2.0, False)
    assert ops.GUARD_HISTORY_MAX == 0.5 / 2e-3
    guard_post(0.25, 1.0, guard_meta("raise"))
    guard_post(0.5, 3.0, guard_meta("raise", "cnf_guard"))
    with pytest.raises(ops.CasprAccuracyError, match=r"error estimate 5.000e-01 > .*; point CNF: .* error estimate 1.000e\+00 > "):
        ops.check_deferred_errors()
    assert ops.GUARD_HISTORY_MAX == 1.0 / 4e-3 and not ops.GUARD_LAST["cnf_guard"]["ok"]
    guard_post(2.0 ** -12, 1.0, guard_meta("raise"))        # estimate 2^-11 < 2e-3: quiet, and the history keeps its maximum
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops.check_deferred_errors()
    assert ops.GUARD_LAST["cnf"]["ok"] and ops.GUARD_LAST["cnf"]["estimate"] == 2.0 ** -11 and ops.GUARD_HISTORY_MAX == 1.0 / 4e-3
    ops.reset_guard()
    assert ops.GUARD_LAST == {} and ops.GUARD_HISTORY_MAX == 0.0


def test_guard_reporter_non_finite_estimate(channels):
    guard_post(float("nan"), 1.0, guard_meta("raise"))
    with pytest.raises(ops.CasprAccuracyError):
        ops.check_deferred_errors()
    assert ops.GUARD_HISTORY_MAX == math.inf and not ops.GUARD_LAST["cnf"]["ok"]


def test_guard_reporter_non_finite_solution_maximum(channels):
    guard_post(2.0 ** -12, float("inf"), guard_meta("raise"))
    ops.check_deferred_errors()
    last = ops.GUARD_LAST["cnf"]
    assert last["bound"] == 1e-3 and last["ok"] and ops.GUARD_HISTORY_MAX == 2.0 ** -11 / 1e-3


def test_guard_keeps_one_ring_for_all_streams(channels, device):
    device.arrives = False
    for _ in range(64):
        ops.guard_track(torch.tensor(0.0), torch.tensor(1.0), guard_meta("raise"))
    assert list(ops._guard.rings) == [None] and len(ops._guard.rings[None]) == 64
    ops.guard_track(torch.tensor(0.0), torch.tensor(1.0), guard_meta("raise"))
    assert len(ops._guard.rings[None]) == 64 and device.events[0].synced == 1


def conv_word(value=0):
    ops._conv_h3.words[KEY] = (i32(value), "its stream")
    return ops._conv_h3.words[KEY][0]


def test_conv_guard_coalesces_copies(channels, device):
    word = conv_word()
    device.arrives = False
    ops._conv_h3.post(KEY)
    ops._conv_h3.post(KEY)                 # a copy is outstanding: no second one, the stream is stale
    assert len(device.events) == 1 and len(ops._conv_h3.rings[KEY]) == 1 and ops._conv_h3.stale == {KEY}
    ops._conv_h3.poll(KEY)                 # not arrived, not waiting: nothing happens
    assert len(device.events) == 1 and ops._conv_h3.stale == {KEY}
    word.fill_(1)                          # the second launch trips
    ops._conv_h3.poll(KEY, wait=False)
    with pytest.raises(CasprHipError, match="conv_split"):
        ops._conv_h3.poll(KEY, wait=True)  # the outstanding copy (clean), then one more fetch for the stale stream
    assert len(device.events) == 2 and ops._conv_h3.stale == set() and ops._conv_h3.rings[KEY] == []
    assert int(word[0]) == 0 and len(device.zeroed) == 1 and device.zeroed[0] is word, "a report zeroes the word"
    ops.check_deferred_errors()
    assert len(device.events) == 2, "nothing launched since: no further copy"


def test_conv_guard_waiting_drain_fetches_for_a_stale_stream_without_a_copy(channels, device):
    conv_word()
    device.arrives = False
    ops._conv_h3.post(KEY)
    ops._conv_h3.post(KEY)
    device.events[0].arrived = True
    ops._conv_h3.poll(KEY)                 # the copy is read; the launch behind it has not been looked at
    assert ops._conv_h3.rings[KEY] == [] and ops._conv_h3.stale == {KEY} and device.zeroed == []
    ops._conv_h3.poll(KEY, wait=True)
    assert len(device.events) == 2 and device.events[1].synced == 1 and ops._conv_h3.stale == set()
    ops._conv_h3.post(KEY)                 # nothing outstanding: a copy of its own
    assert len(device.events) == 3 and ops._conv_h3.stale == set()
    assert len(device.allocated) == 1, "one pinned word serves them all"


def test_conv_guard_trip_then_clean_launch_then_drain(channels, device):
    word = conv_word()
    device.arrives = False
    ops._conv_h3.post(KEY)
    word.fill_(1)                          # tripped behind the outstanding copy; a clean launch follows
    ops._conv_h3.post(KEY)
    ops._conv_h3.post(KEY)
    with pytest.raises(CasprHipError, match='conv_split="bf16x6"'):
        ops.check_deferred_errors()
    ops.check_deferred_errors()


def test_an_earlier_channels_error_leaves_the_later_channels_queued(channels):
    ops._steps.post(KEY, i32(2), (64, 1e-5))
    ops._team.post(KEY, i32(1))
    with pytest.raises(CasprHipError, match="team barrier") as e:
        ops.check_deferred_errors()
    assert not isinstance(e.value, ops.CasprAccuracyError) and len(ops._steps.rings[KEY]) == 1
    with pytest.raises(ops.CasprAccuracyError, match=r"2 frame\(s\) capped at 64 steps"):
        ops.check_deferred_errors()
    ops.check_deferred_errors()
