"""The case table and the recorder for the dispatch test of the pointwise conv front-end (caspr_amd/ops.py: conv1x1, conv1x1_gn,
conv1x1_gn_early_ok, conv1x1_gn_early, conv1x1_gn_tail_beside): test_conv_dispatch.py compares the transcript of every case with
tests/golden/conv_dispatch_parent.json.  Everything runs on the CPU; no kernel is loaded.

transcript(case) calls the front-end with the library replaced by a recorder and returns what it did, in order, one list per event:

    [entry name, argument, ...]                 a call into the library (*_bytes entries answer 4096, every other entry 0)
    ["pack", "x3" | "xw" | "xh", stream]        a request for one of the weight's lazily built packs, and the current stream then
    ["h3", "enter" | "leave"]                   the scope of the f16x3 status word around a launch (ops._conv_h3_launch)
    ["enter" | "leave", stream]                 with torch.cuda.stream(stream)
    ["record", event, stream], ["wait_event", stream, event], ["wait_stream", stream, other], ["record_stream", tensor, stream]
    ["on_early", tensor]                        conv1x1_gn_early's callback
    ["raise", type, text]                       the exception the call ended with
    ["return", [shape, row stride] | null ...]  what it returned (a bool for conv1x1_gn_early_ok)
    ["end", n, key, ...]                        by how much CONV_ROUTE_COUNT["h3w"] advanced, and the keys ops.timed recorded under
                                                (TIMING = 2; its events are in the lines above)

A pointer argument is named after the tensor it points into -- the role of an input ("x", "bias", "pw.xw.main", ...), "ret[i]" for
the i-th returned tensor, "ws" for the workspace, "word" for the status word, "null" -- so that no address enters the transcript;
scalars stand as they are.  Events are numbered in the order of their creation ("ev0", ...), streams are "main" and "tail".

The golden file is this module's output ON THE COMMIT BEFORE the front-end was given one route table, never on the code under test:
    python tests/conv_dispatch_cases.py tests/golden/conv_dispatch_parent.json
run with that commit's caspr_amd/ops.py in the tree.
"""
import contextlib
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from caspr_amd import lib, ops, train_ops  # noqa: E402

WORD = 0x40              # the fixed status word of the stubbed _conv_h3_launch
LOW = {"_X6W_MIN_CIN": 32, "_X6W_MIN_ROWS": 128}       # the thresholds the GPU tests lower to reach the wide kernel with small layers
WIDE = ((1600, 576), (1600, 1600), (512, 512))         # (Cout, Cin): the persistent 512-channel kernel's layers at the default thresholds
LAYERS = WIDE + ((1024, 128), (256, 256), (128, 64), (64, 32))

CASES = []
_names = set()


def _add(fn, layer, P, B=2, low=False, x6=True, x6w=True, cs="bf16x6", **kw):
    """One call of ops.<fn> on a (Cout, Cin) layer.  cs: ops.CONV_SPLIT.  kw: the call's own keywords; a tensor argument is asked for by
    naming it True (bbias, in_scale -- with in_shift --, out), tail_stream by True, plus
    x_cols (the channels of x's rows, default Cin), x_ld (their stride), capturing (what torch.cuda.is_current_stream_capturing says)."""
    name = "%s:%dx%d:B%d:P%d" % (fn, layer[0], layer[1], B, P) + (":low" if low else "") + ("" if x6 else ":x6off") + ("" if x6w else ":x6woff")
    name += ":" + cs + "".join(":%s=%s" % (k, v) for k, v in kw.items())
    if name in _names:
        return
    _names.add(name)
    CASES.append(SimpleNamespace(name=name, fn=fn, cout=layer[0], cin=layer[1], B=B, P=P, low=low, x6=x6, x6w=x6w, cs=cs, kw=kw))


def _build():
    both = ("bf16x6", "f16x3")
    for fn in ("conv1x1", "conv1x1_gn"):
        # every layer at every row count that changes the route; both forms of the wide kernel where it is reached
        for layer in LAYERS:
            for P in (1024, 896, 100):
                for cs in both if layer in WIDE and P == 1024 else both[:1]:
                    _add(fn, layer, P, cs=cs)
            for cs in both if layer in WIDE else both[:1]:
                _add(fn, layer, 128, low=True, cs=cs)
        _add(fn, (1600, 576), 100, low=True)
        _add(fn, (1600, 576), 896, low=True, cs="f16x3")
        for P in (1024, 128):                              # x6w_ok without x6_gn_ok: conv1x1 + gn_stats, the conv on the wide kernel with G = 0
            for cs in both:
                _add(fn, (512, 32), P, low=True, cs=cs)
        _add(fn, (512, 32), 1024)
        # the switches
        for layer in ((1600, 576), (256, 256)):
            _add(fn, layer, 1024, x6=False, cs="f16x3")
            _add(fn, layer, 1024, x6w=False, cs="f16x3")
            _add(fn, layer, 1024, cs="f16x4")                  # misspelt
            _add(fn, layer, 1024, cs="f16x4", split="bf16x6")
        _add(fn, (1600, 576), 1024, cs="f16x3", split="bf16x6")
        _add(fn, (1600, 576), 1024, cs="bf16x6", split="f16x3")
        _add(fn, (1600, 576), 100, cs="f16x4")
        # the fused input transform
        for layer in ((1600, 576), (256, 256)):
            for k in (8, 4):
                _add(fn, layer, 1024, cs="f16x3", in_scale=True, in_relu=True, in_relu_from=k)
            _add(fn, layer, 1024, cs="f16x3", bbias=True, in_scale=True, out=True, x_ld=1608)
        _add(fn, (64, 32), 1024, bbias=True, in_scale=True, in_relu=True, in_relu_from=4, out=True, x_ld=1608)
        for layer in ((1600, 576), (64, 32)):
            _add(fn, layer, 1024, x_cols=layer[1] - 4)        # rows narrower than Cin
            _add(fn, layer, 1024, x_cols=layer[1] - 3, x_ld=layer[1])      # ... but the buffer behind them is wide enough
    _add("conv1x1_train", (1600, 576), 1024, cs="f16x3")
    _add("conv1x1_train", (256, 256), 1024, cs="f16x3", act=1)
    for layer in ((1600, 576), (256, 256), (64, 32)):
        for cs in both:
            _add("conv1x1", layer, 1024, cs=cs, act=1)
            _add("conv1x1", layer, 1024, cs=cs, row_invariant=True)
    _add("conv1x1", (1600, 576), 1024, cs="f16x4", act=1)  # off the wide kernel: the misspelt switch is not looked at
    _add("conv1x1", (1600, 576), 1024, act=1, row_invariant=True)
    # conv1x1_gn's own
    for layer in ((1600, 576), (512, 512), (1024, 128), (256, 256), (64, 32)):
        for cs in both if layer in WIDE else both[:1]:
            _add("conv1x1_gn", layer, 1024, B=4, cs=cs, pool=2)
            _add("conv1x1_gn", layer, 1024, B=4, cs=cs, pool=2, want_max=True, want_moments=True, bbias=True, in_scale=True)
    _add("conv1x1_gn", (1600, 576), 128, B=4, low=True, cs="f16x3", pool=4)
    _add("conv1x1_gn", (512, 32), 128, B=4, low=True, cs="f16x3", pool=2)
    for layer in ((1600, 576), (64, 32)):
        _add("conv1x1_gn", layer, 1024, B=4, pool=3)
        _add("conv1x1_gn", layer, 1024, B=4, pool=0)
        _add("conv1x1_gn", layer, 1024, B=4, pool=3, cs="f16x4")
    for layer in ((1600, 576), (256, 256), (64, 32)):
        for cs in both if layer in WIDE else both[:1]:
            _add("conv1x1_gn", layer, 1024, cs=cs, want_max=True)
            _add("conv1x1_gn", layer, 1024, cs=cs, want_moments=True, groups=32)
            _add("conv1x1_gn", layer, 1024, cs=cs, write=False)
            _add("conv1x1_gn", layer, 1024, cs=cs, write=False, out=True, want_max=True)
        _add("conv1x1_gn", layer, 1024, cs="f16x3", groups=7)          # C % groups != 0: conv1x1 + gn_stats
        _add("conv1x1_gn", layer, 1024, cs="f16x4", groups=7)
        _add("conv1x1_gn", layer, 1024, cs="f16x4", x_cols=layer[1] - 4)  # the narrow rows are reported before the misspelt switch
    # conv1x1_gn_early_ok / conv1x1_gn_early
    for layer, P, low in (((1600, 576), 1024, False), ((1600, 576), 896, False), ((1600, 576), 128, True), ((512, 512), 1024, False),
                          ((1024, 128), 1024, False), ((1024, 128), 128, True), ((1024, 32), 128, True), ((256, 256), 1024, False)):
        _add("conv1x1_gn_early_ok", layer, P, low=low, early_channels=64)
        _add("conv1x1_gn_early", layer, P, low=low, cs="f16x3", tail_stream=True)
    for kw in (dict(early_channels=100), dict(early_channels=101), dict(groups=7, early_channels=1), dict(cs="f16x4", early_channels=1),
               dict(x6w=False, early_channels=1), dict(x6=False, early_channels=1)):
        _add("conv1x1_gn_early_ok", (1600, 576), 1024, **kw)
    _add("conv1x1_gn_early_ok", (2048, 512), 1024, groups=2, early_channels=513)
    for cs in both:
        for tail in (False, True):
            for reserve in (0, 32):
                _add("conv1x1_gn_early", (1600, 576), 1024, cs=cs, tail_stream=tail, reserve_cus=reserve)
        _add("conv1x1_gn_early", (1600, 1600), 1024, cs=cs, tail_stream=True, in_scale=True, in_relu=True, in_relu_from=8)
        _add("conv1x1_gn_early", (1024, 128), 128, low=True, cs=cs)
    _add("conv1x1_gn_early", (1600, 576), 1024, cs="f16x4", tail_stream=True)
    _add("conv1x1_gn_early", (1600, 576), 1024, groups=7)
    _add("conv1x1_gn_early", (1600, 576), 1024, in_scale=True, in_relu=True, in_relu_from=4)        # not looked at: as the parent
    # conv1x1_gn_tail_beside
    for cs in both:
        for tail in (False, True):
            for pool in (1, 2):
                _add("conv1x1_gn_tail_beside", (1600, 576), 1024, B=4, cs=cs, tail_stream=tail, pool=pool)
        _add("conv1x1_gn_tail_beside", (1600, 1600), 1024, cs=cs, tail_stream=True, bbias=True, in_scale=True, in_relu=True, in_relu_from=8)
        _add("conv1x1_gn_tail_beside", (512, 512), 1024, cs=cs, tail_stream=True)          # no remainder
        _add("conv1x1_gn_tail_beside", (1600, 576), 1024, cs=cs, tail_stream=True, capturing=True)
    for layer, P, low in (((1024, 128), 1024, False), ((256, 256), 1024, False), ((1600, 576), 896, False), ((1600, 32), 128, True),
                          ((1600, 576), 128, True)):
        _add("conv1x1_gn_tail_beside", layer, P, low=low, cs="f16x3", tail_stream=True)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, tail_stream=True, in_relu_from=4)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, tail_stream=True, groups=7)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, B=4, tail_stream=True, pool=3)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, tail_stream=True, x6w=False)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, tail_stream=True, x6=False)
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, tail_stream=True, cs="f16x4")
    _add("conv1x1_gn_tail_beside", (1600, 576), 1024, cs="f16x4")


_build()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------
# the stand-ins
# ---------------------------------------------------------------------------------------------
class FakeWeight:
    """What the front-end reads of a PackedWeight: the three flags by the formulas of PackedWeight.__init__ at the thresholds of the
    moment, and a tensor of its own per pack.  asked(which) hears of every request for a lazily built pack: the real one allocates
    and launches its pack kernels on the current stream at the first request."""

    def __init__(self, cout, cin, asked=lambda which: None):
        self.cout, self.cin, self.asked = cout, cin, asked
        self.x6_ok = cin % 32 == 0 and cin >= ops._X6_MIN_CIN and cout % 4 == 0 and cout >= 128
        self.x6_gn_ok = cin % 32 == 0 and cin >= ops._X6_GN_MIN_CIN and cout % 4 == 0 and cout >= 128
        self.x6w_ok = cin % 32 == 0 and cin >= ops._X6W_MIN_CIN and cout % 4 == 0 and cout >= 512
        tail = cout % 512 != 0
        self.data, self._x3 = torch.empty(4), torch.empty(4)
        self._xw = (torch.empty(4), torch.empty(4) if tail else None)
        self._xh = (torch.empty(4), torch.empty(4) if tail else None)

    def x3(self):
        self.asked("x3")
        return self._x3

    def xw(self):
        self.asked("xw")
        return self._xw

    def xh(self):
        self.asked("xh")
        return self._xh

    def roles(self):
        named = {"pw.data": self.data, "pw.x3": self._x3, "pw.xw.main": self._xw[0], "pw.xw.tail": self._xw[1], "pw.xh.main": self._xh[0],
                 "pw.xh.tail": self._xh[1]}
        return {t.data_ptr(): role for role, t in named.items() if t is not None}


class FakeStream:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def wait_event(self, ev):
        self.log.append(["wait_event", self.name, ev.name])

    def wait_stream(self, other):
        self.log.append(["wait_stream", self.name, other.name])


def _raw(v):
    """An argument as recorded: a pointer as ("ptr", address) until the roles are known."""
    if isinstance(v, ctypes.c_void_p):
        return ("ptr", v.value)
    if v is None:
        return ("ptr", None)
    if isinstance(v, torch.Tensor):
        return ("ptr", v.data_ptr())
    assert isinstance(v, (int, float, str)), v
    return v


def _describe(t):
    return None if t is None else [list(t.shape), t.stride(1) if t.dim() == 3 else t.stride(0)]


def transcript(case):
    """Run one case against the recorder -> its transcript (see the module's docstring)."""
    log = []
    state = SimpleNamespace(events=0, ws=None)
    main, tail = FakeStream(log, "main"), FakeStream(log, "tail")
    streams = [main]

    class Library:
        def __getattr__(self, name):
            def entry(*args):
                log.append([name] + [_raw(a) for a in args])
                return 4096 if name.endswith("_bytes") else 0
            return entry

    class Event:
        def __init__(self, enable_timing=False):
            self.name = "ev%d" % state.events
            state.events += 1

        def record(self, stream=None):
            log.append(["record", self.name, (stream or streams[-1]).name])

    @contextlib.contextmanager
    def on_stream(stream):
        log.append(["enter", stream.name])
        streams.append(stream)
        try:
            yield
        finally:
            streams.pop()
            log.append(["leave", stream.name])

    @contextlib.contextmanager
    def h3_launch(x):
        ops.CONV_ROUTE_COUNT["h3w"] += 1
        log.append(["h3", "enter"])
        yield ctypes.c_void_p(WORD)
        log.append(["h3", "leave"])

    def workspace(nbytes, device):
        if state.ws is None:
            state.ws = torch.empty(nbytes, dtype=torch.uint8)
        return state.ws

    def chk_rows(t):
        return 0 if t is None else t.stride(1)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "load", Library)
        for mod in (ops, train_ops):                     # train_ops took its copies of these names at import
            mp.setattr(mod, "_chk_f32", lambda *ts: None)
            mp.setattr(mod, "_chk_rows", chk_rows)
            mp.setattr(mod, "_stream", lambda: ctypes.c_void_p(0))
            mp.setattr(mod, "_workspace", workspace)
        mp.setattr(ops, "_conv_h3_launch", h3_launch)
        mp.setattr(torch.cuda, "current_stream", lambda device=None: streams[-1])
        mp.setattr(torch.cuda, "stream", on_stream)
        mp.setattr(torch.cuda, "Event", Event)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: bool(case.kw.get("capturing", False)))
        mp.setattr(torch.Tensor, "record_stream", lambda self, stream: log.append(["record_stream", _raw(self), stream.name]))
        for name, value in (LOW if case.low else {}).items():
            mp.setattr(ops, name, value)
        mp.setattr(ops, "CONV_BF16X6", case.x6)
        mp.setattr(ops, "CONV_X6W", case.x6w)
        mp.setattr(ops, "CONV_SPLIT", case.cs)
        mp.setattr(ops, "TIMING", 2)
        mp.setattr(ops, "TIMERS", {})
        mp.setitem(ops.CONV_ROUTE_COUNT, "h3w", 0)

        kw = dict(case.kw)
        B, P, cin, cout = case.B, case.P, case.cin, case.cout
        pw = FakeWeight(cout, cin, lambda which: log.append(["pack", which, streams[-1].name]))
        cols = kw.pop("x_cols", cin)
        t = SimpleNamespace(x=torch.empty(B, P, kw.pop("x_ld", cols))[:, :, :cols], bias=torch.empty(cout), gamma=torch.empty(cout), beta=torch.empty(cout))
        if kw.pop("bbias", False):
            t.bbias = kw["bbias"] = torch.empty(B, cout)
        if kw.pop("in_scale", False):
            t.in_scale, t.in_shift = kw["in_scale"], kw["in_shift"] = torch.empty(B, cin), torch.empty(B, cin)
        if kw.pop("out", False):
            t.out = kw["out"] = torch.empty(B, P, 1608)[:, :, :(cout + 3) // 4 * 4]
        if "tail_stream" in kw:
            kw["tail_stream"] = tail if kw["tail_stream"] else None
        kw.pop("capturing", None)
        roles = pw.roles()
        roles.update({v.data_ptr(): k for k, v in vars(t).items()})
        try:
            if case.fn == "conv1x1_gn_early_ok":
                ret = ops.conv1x1_gn_early_ok(pw, B, P, kw.pop("groups", 16), **kw)
            elif case.fn in ("conv1x1", "conv1x1_train"):
                ret = getattr(ops, case.fn)(pw, t.bias, t.x, **kw)
            elif case.fn == "conv1x1_gn":
                ret = ops.conv1x1_gn(pw, t.bias, t.x, t.gamma, t.beta, **kw)
            elif case.fn == "conv1x1_gn_early":
                ret = ops.conv1x1_gn_early(pw, t.bias, t.x, t.gamma, t.beta, lambda pmax: log.append(["on_early", _raw(pmax)]), **kw)
            else:
                ret = ops.conv1x1_gn_tail_beside(pw, t.bias, t.x, t.gamma, t.beta, **kw)
        except Exception as e:        # noqa: BLE001 -- whatever it is, it is the transcript's last word
            ret = None
            log.append(["raise", type(e).__name__, str(e)])
        else:
            if isinstance(ret, torch.Tensor):
                roles.setdefault(ret.data_ptr(), "ret")
                log.append(["return", _describe(ret)])
            elif isinstance(ret, tuple):
                for i, r in enumerate(ret):
                    if r is not None:
                        roles.setdefault(r.data_ptr(), "ret[%d]" % i)
                log.append(["return"] + [_describe(r) for r in ret])
            else:
                log.append(["return", ret])
        log.append(["end", ops.CONV_ROUTE_COUNT["h3w"]] + list(ops.TIMERS))
    roles[None] = "null"
    roles[WORD] = "word"
    if state.ws is not None:
        roles[state.ws.data_ptr()] = "ws"
    return [[roles.get(v[1], "unknown") if isinstance(v, tuple) else v for v in line] for line in log]


def dump(path):
    """All transcripts as one JSON list, a line per event, each case behind its ["case", name] line."""
    lines = []
    for c in CASES:
        lines.append(["case", c.name])
        lines.extend(transcript(c))
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(line, separators=(",", ":")) for line in lines) + "\n]\n")


def load(path):
    """-> {case name: transcript}"""
    out = {}
    with open(path) as f:
        for line in json.load(f):
            if line[0] == "case":
                cur = out[line[1]] = []
            else:
                cur.append(line)
    return out


if __name__ == "__main__":
    dump(sys.argv[1])
    print("%d cases -> %s" % (len(CASES), sys.argv[1]))
