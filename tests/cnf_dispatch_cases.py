"""The case table and the recorder for the dispatch test of the point-CNF front-end (caspr_amd/ops.py: cnf_rk4, cnf_dopri5;
caspr_amd/train_ops.py: cnf_train_fwd, cnf_sample_tape, cnf_sample_tape_frames, cnf_sample_tape_h3, cnf_sample_tape_h3_frames;
caspr_amd/train/flow_grad.py: _sample_tape_route): test_cnf_dispatch.py compares the transcript of every case with
tests/golden/cnf_dispatch_parent.json.  Everything runs on the CPU; no kernel is loaded.

transcript(case) calls the front-end with the library replaced by a recorder and returns what it did, in order, one list per event:

    [entry name, argument, ...]                 a call into the library (*_bytes entries answer 4096, every other entry 0)
    ["h3", "enter" | "post" | "leave"]          the scope of the f16x3 range guard's status word around a launch (ops._cnf_h3.on), and
                                                the post of the word behind it
    ["record", event, stream]                   a timer's event (TIMING = 2)
    ["raise", type, text]                       the exception the call ended with
    ["return", [pointer, shape] | value ...]    what it returned; a trace dict as ["info", [key, storage, offset, shape] | [key, str] ...]
    ["end", key, ...]                           the keys ops.timed recorded under

A pointer argument is named after the tensor it points into -- the role of an input ("y", "hyper", "w1x", "w1h", "t_end", ...),
"ret[i]" for the i-th returned tensor, "ws" for the workspace, "word" for the status word, "null", and "new:<dtype>:<shape>" for a
tensor the call allocated and kept to itself (cnf_dopri5's trace and counters) -- so that no address enters the transcript; scalars
stand as they are.  Events are numbered in the order of their creation ("ev0", ...), the stream is "main".  The argument checks
(_chk_f32, _chk_frame_table and every check of the CNF functions) are the front-end's own: their texts are part of what is pinned.
Every erroneous case violates ONE condition: the order of the checks inside a function is not pinned, the exception is.

The golden file is this module's output ON THE COMMIT BEFORE the front-end was given one route table, never on the code under test:
    python tests/cnf_dispatch_cases.py tests/golden/cnf_dispatch_parent.json
run with that commit's caspr_amd/ops.py, caspr_amd/train_ops.py and caspr_amd/train/flow_grad.py in the tree.
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
from caspr_amd.train import flow_grad  # noqa: E402

BT = 2
LDH = 3080               # hyper's row width: wider than the 3078 floats the kernels read, so that the ld argument is not that constant
TRAIN = ("cnf_train_fwd", "cnf_sample_tape", "cnf_sample_tape_frames", "cnf_sample_tape_h3", "cnf_sample_tape_h3_frames")
FRAMES = ("cnf_sample_tape_frames", "cnf_sample_tape_h3_frames")
PACKS = ("none", "x6", "x6h3", "h3", "w1x", "w2x", "x6w1h")      # which of w1x / w2x / w1h / w2h a cnf_rk4 / cnf_dopri5 call hands over
E_BAD = ("e_only", "logp_only", "e_shape", "logp_shape")        # the violations that start from a call with e and logp

CASES = []
_names = set()


def _add(fn, n, **kw):
    """One call of <fn> on BT frames of n points.  kw (all optional; a tensor argument is asked for by naming it True):
    packs (PACKS; cnf_rk4 / cnf_dopri5), e (e and logp), narrow, reverse, mbn (mbn_in and mbn_out), table (steps as a (BT,) tensor), order,
    max_steps, out, ys (ys and ka), return_trace, capturing (what torch.cuda.is_current_stream_capturing says), split (ops.CNF_TAPE_SPLIT),
    solve (the packs as flow_grad._SolvePacks), bad (the one condition the call violates: _violate)."""
    name = "%s:n%d" % (fn, n) + "".join(":%s=%s" % (k, v) for k, v in kw.items())
    if name in _names:
        return
    _names.add(name)
    CASES.append(SimpleNamespace(name=name, fn=fn, n=n, kw=kw))


def _build():
    # cnf_rk4: the pack combinations against e / logp, narrow and n around the f16x3 workgroup's 128 points, the direction with them
    for packs in PACKS[:6]:
        for e in (False, True):
            for narrow in (False, True):
                for n in (127, 128):
                    _add("cnf_rk4", n, packs=packs, e=e, narrow=narrow, reverse=(n == 128) != narrow)
            for n in (64, 200):
                _add("cnf_rk4", n, packs=packs, e=e, reverse=True)
            _add("cnf_rk4", 128, packs=packs, e=e, mbn=True)
        _add("cnf_rk4", 128, packs=packs, reverse=True)
        _add("cnf_rk4", 128, packs=packs, reverse=False, narrow=True)
        _add("cnf_rk4", 128, packs=packs, reverse=True, narrow=True, mbn=True)
    _add("cnf_rk4", 128, packs="x6w1h", reverse=True)               # one h pack only: where it goes without them
    for bad in ("y_shape", "y_f64", "y_noncontig", "hyper_rows", "e_only", "logp_only", "e_shape", "logp_shape", "mbn_in_size", "mbn_out_size"):
        _add("cnf_rk4", 128, packs="x6", reverse=True, e=bad in E_BAD, bad=bad)
    _add("cnf_rk4", 128, packs="x6", reverse=True, bad="w0_shape")        # the hidden width is C's to refuse: H = w0's rows goes through
    _add("cnf_dopri5", 128, packs="x6", reverse=True, bad="w0_shape")
    for bad in ("h3_size", "h3_dtype"):
        _add("cnf_rk4", 128, packs="x6h3", reverse=True, bad=bad)
        _add("cnf_rk4", 127, packs="x6h3", reverse=True, bad=bad)   # not looked at off the f16x3 route
    # ... with a step table
    for packs, n in (("x6", 64), ("x6", 128), ("x6h3", 127), ("x6h3", 128), ("x6h3", 200)):
        _add("cnf_rk4", n, packs=packs, reverse=True, table=True)
        _add("cnf_rk4", n, packs=packs, reverse=True, table=True, order=True, out=True, max_steps=7)
    for packs in ("x6", "x6h3"):
        _add("cnf_rk4", 128, packs=packs, reverse=False, table=True, order=True)
        _add("cnf_rk4", 128, packs=packs, reverse=True, table=True, out=True, mbn=True)
        _add("cnf_rk4", 128, packs=packs, reverse=True, table=True, narrow=True, order=True)
        _add("cnf_rk4", 128, packs=packs, reverse=False, table=True, narrow=True)
        for max_steps in (1, 4096, 4097, 0):
            _add("cnf_rk4", 128, packs=packs, reverse=True, table=True, max_steps=max_steps)
    for packs in ("none", "h3", "w1x", "w2x"):
        _add("cnf_rk4", 128, packs=packs, reverse=True, table=True)         # a table needs the x6 packs, f16x3 or not
    _add("cnf_rk4", 128, packs="x6", reverse=True, table=True, e=True)
    for bad in ("steps_dtype", "steps_len", "steps_noncontig", "steps_2d", "steps_device", "order_dtype", "order_len", "order_noncontig",
                "order_list", "out_shape", "out_f64", "h3_size"):
        _add("cnf_rk4", 128, packs="x6h3", reverse=True, table=True, order=True, out=True, bad=bad)
    _add("cnf_rk4", 128, packs="x6", reverse=True, order=True)
    _add("cnf_rk4", 128, packs="x6", reverse=True, max_steps=8)
    _add("cnf_rk4", 128, packs="x6h3", reverse=True, out=True)
    # cnf_dopri5
    for packs in ("x6", "x6h3"):
        for n in (127, 128):
            for e in (False, True):
                for return_trace in (False, True):
                    _add("cnf_dopri5", n, packs=packs, e=e, reverse=not e, return_trace=return_trace)
        _add("cnf_dopri5", 200, packs=packs, reverse=True, return_trace=True, mbn=True, max_attempts=3)
        _add("cnf_dopri5", 64, packs=packs, reverse=False, mbn=True)
    _add("cnf_dopri5", 128, packs="x6w1h", reverse=True, return_trace=True)
    for packs in ("none", "h3", "w1x", "w2x"):
        _add("cnf_dopri5", 128, packs=packs, reverse=True)
    for bad in ("y_shape", "y_f64", "hyper_rows", "e_only", "logp_only", "e_shape", "logp_shape", "mbn_in_size", "mbn_out_size", "rtol_0", "rtol_inf",
                "atol_0", "atol_nan", "t_end_0", "t_end_inf", "max_attempts_0", "h3_size", "h3_dtype", "requires_grad"):
        _add("cnf_dopri5", 128, packs="x6h3", reverse=True, e=bad in E_BAD, bad=bad)
    for bad in ("h3_size", "h3_dtype"):
        _add("cnf_dopri5", 127, packs="x6h3", reverse=True, bad=bad)
    _add("cnf_dopri5", 128, packs="x6h3", reverse=True, bad="requires_grad", no_grad=True)
    _add("cnf_dopri5", 128, packs="x6h3", reverse=True, capturing=True)
    _add("cnf_dopri5", 128, packs="x6", reverse=True, capturing=True)
    # the five wrappers of the training tier
    for fn in TRAIN:
        h3, frames = "_h3" in fn, fn in FRAMES
        for n in (128, 200) + (() if h3 else (64, 127)):
            _add(fn, n)
        if h3:
            _add(fn, 127)                               # below the 128-point workgroup
        bad = ["y_shape", "y_f64", "hyper_rows", "hyper_width", "tcol_short", "w0_shape", "w3_shape", "b0_size", "b1_size", "b2_size", "b3_size",
               "pack1_missing", "pack2_missing", "pack1_size", "pack2_size", "pack_dtype", "t_end_numel"]
        if fn == "cnf_train_fwd":
            bad += ["e_shape", "logp_shape"]
        if frames:
            _add(fn, 128, order=True)
            _add(fn, 128, ys=True)
            _add(fn, 128, order=True, ys=True, max_steps=1)
            _add(fn, 128, max_steps=4096)
            _add(fn, 128, max_steps=4097)
            _add(fn, 128, max_steps=0)
            bad += ["steps_dtype", "steps_len", "steps_noncontig", "steps_int", "steps_device", "order_dtype", "order_len", "order_noncontig",
                    "ys_shape", "ka_shape", "ys_noncontig", "ka_f64"]
        else:
            _add(fn, 128, steps=0)
            _add(fn, 128, steps=-1)
        for b in bad:
            _add(fn, 128, **(dict(order=True, ys=True) if frames else {}), bad=b)
    # flow_grad._sample_tape_route
    for solve in (False, True):
        for n in (127, 128):
            for split in ("bf16x6", "f16x3", "f16x4"):
                _add("_sample_tape_route", n, solve=solve, split=split)


_build()
BY_NAME = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------
# the stand-ins
# ---------------------------------------------------------------------------------------------
def _violate(t, n, bad, fn):
    """Break ONE condition of the call whose tensors are t."""
    f32, nb = torch.float32, 4096
    tape = (4 if fn in FRAMES else 3, 4, BT, n, 3)
    new = {
        "y_shape": ("y", lambda: torch.empty(BT, n, 4)), "y_f64": ("y", lambda: torch.empty(BT, n, 3, dtype=torch.float64)),
        "y_noncontig": ("y", lambda: torch.empty(BT, 3, n).transpose(1, 2)), "requires_grad": ("y", lambda: torch.empty(BT, n, 3, requires_grad=True)),
        "hyper_rows": ("hyper", lambda: torch.empty(BT + 1, LDH)), "hyper_width": ("hyper", lambda: torch.empty(BT, 3077)),
        "tcol_short": ("tcol", lambda: torch.empty(3077)),
        "e_only": ("logp", lambda: None), "logp_only": ("e", lambda: None),
        "e_shape": ("e", lambda: torch.empty(BT, n + 1, 3)), "logp_shape": ("logp", lambda: torch.empty(BT, n)),
        "mbn_in_size": ("mbn_in", lambda: torch.empty(11)), "mbn_out_size": ("mbn_out", lambda: torch.empty(13)),
        "w0_shape": ("w0", lambda: torch.empty(511, 3)), "w3_shape": ("w3", lambda: torch.empty(3, 511)),
        "b0_size": ("b0", lambda: torch.empty(511)), "b1_size": ("b1", lambda: torch.empty(513)), "b2_size": ("b2", lambda: torch.empty(511)),
        "b3_size": ("b3", lambda: torch.empty(4)),
        "h3_size": ("w2h", lambda: torch.empty(nb - 1, dtype=torch.uint8)), "h3_dtype": ("w1h", lambda: torch.empty(nb, dtype=torch.int8)),
        "pack1_missing": ("w1", lambda: None), "pack2_missing": ("w2", lambda: None),
        "pack1_size": ("w1", lambda: torch.empty(nb + 1, dtype=torch.uint8)), "pack2_size": ("w2", lambda: torch.empty(nb - 1, dtype=torch.uint8)),
        "pack_dtype": ("w2", lambda: torch.empty(nb, dtype=torch.int8)),
        "t_end_numel": ("t_end", lambda: torch.empty(2)),
        "steps_dtype": ("steps", lambda: torch.empty(BT, dtype=torch.int64)), "steps_len": ("steps", lambda: torch.empty(BT + 1, dtype=torch.int32)),
        "steps_noncontig": ("steps", lambda: torch.empty(2 * BT, dtype=torch.int32)[::2]), "steps_2d": ("steps", lambda: torch.empty(BT, 1, dtype=torch.int32)),
        "steps_int": ("steps", lambda: 5), "steps_device": ("steps", lambda: torch.empty(BT, dtype=torch.int32, device="meta")),
        "order_dtype": ("order", lambda: torch.empty(BT, dtype=f32)), "order_len": ("order", lambda: torch.empty(BT - 1, dtype=torch.int32)),
        "order_noncontig": ("order", lambda: torch.empty(2 * BT, dtype=torch.int32)[::2]), "order_list": ("order", lambda: [1, 0]),
        "out_shape": ("out", lambda: torch.empty(BT, n + 1, 3)), "out_f64": ("out", lambda: torch.empty(BT, n, 3, dtype=torch.float64)),
        "ys_shape": ("ys", lambda: torch.empty(tape[0] + 1, *tape[1:])), "ka_shape": ("ka", lambda: torch.empty(*tape[:3], n + 1, 3)),
        "ys_noncontig": ("ys", lambda: torch.empty(*tape[:4], 6)[..., ::2]), "ka_f64": ("ka", lambda: torch.empty(tape, dtype=torch.float64)),
    }
    scalars = {"rtol_0": ("rtol", 0.0), "rtol_inf": ("rtol", float("inf")), "atol_0": ("atol", 0.0), "atol_nan": ("atol", float("nan")),
               "t_end_0": ("t_end", 0.0), "t_end_inf": ("t_end", float("inf")), "max_attempts_0": ("max_attempts", 0)}
    if bad in scalars:
        setattr(t, *scalars[bad])
    else:
        name = new[bad][0]
        setattr(t, name + ("h" if "_h3" in fn else "x") if name in ("w1", "w2") else name, new[bad][1]())


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


def _returned(r):
    if isinstance(r, torch.Tensor):
        return [_raw(r), list(r.shape)]
    if isinstance(r, dict):
        return ["info"] + [[k, v] if isinstance(v, str) else [k, ("ptr", v.untyped_storage().data_ptr()), v.storage_offset(), list(v.shape)] for k, v in r.items()]
    return r


def transcript(case):
    """Run one case against the recorder -> its transcript (see the module's docstring)."""
    log = []
    state = SimpleNamespace(events=0, ws=None, new=[])
    main = SimpleNamespace(name="main")
    word = torch.zeros(1, dtype=torch.int32)
    kw = dict(case.kw)
    n, fn = case.n, case.fn

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
            log.append(["record", self.name, (stream or main).name])

    class Channel:
        """ops._cnf_h3: the scope of the status word, and the post behind the launch."""

        @contextlib.contextmanager
        def on(self, device):
            log.append(["h3", "enter"])
            yield SimpleNamespace(word=word, live=True, post=lambda src=None, meta=None: log.append(["h3", "post", _raw(src)]))
            log.append(["h3", "leave"])

    def workspace(nbytes, device):
        if state.ws is None:
            state.ws = torch.empty(nbytes, dtype=torch.uint8)
        return state.ws

    def keeping(make):
        def made(*args, **kwargs):
            state.new.append(make(*args, **kwargs))          # kept alive: no address is handed out twice within a case
            return state.new[-1]
        return made

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(lib, "load", Library)
        for mod in (ops, train_ops):                     # train_ops took its copies of these names at import
            mp.setattr(mod, "_stream", lambda: ctypes.c_void_p(0), raising=False)
            mp.setattr(mod, "_workspace", workspace, raising=False)
        mp.setattr(ops, "_cnf_h3", Channel())
        mp.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
        mp.setattr(torch.cuda, "current_device", lambda: None)         # a CPU tensor's device index: _on_current_device passes
        mp.setattr(torch.cuda, "current_stream", lambda device=None: main)
        mp.setattr(torch.cuda, "Event", Event)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: bool(case.kw.get("capturing", False)))
        mp.setattr(ops, "CNF_TAPE_SPLIT", kw.pop("split", "bf16x6"))
        mp.setattr(ops, "TIMING", 2)
        mp.setattr(ops, "TIMERS", {})

        pack = lambda: torch.empty(4096, dtype=torch.uint8)         # noqa: E731
        t = SimpleNamespace(y=torch.empty(BT, n, 3), hyper=torch.empty(BT, LDH), tcol=torch.empty(3078), w0=torch.empty(512, 3), b0=torch.empty(512),
                            b1=torch.empty(512), b2=torch.empty(512), w3=torch.empty(3, 512), b3=torch.empty(3))
        for k in ("e", "logp", "mbn_in", "mbn_out", "order", "out", "ys", "ka", "w1x", "w2x", "w1h", "w2h"):
            setattr(t, k, None)
        if fn in ("cnf_rk4", "cnf_dopri5"):
            packs = kw.pop("packs")
            t.w1p, t.w2p = torch.empty(4), torch.empty(4)
            if packs in ("x6", "x6h3", "w1x", "x6w1h"):
                t.w1x = pack()
            if packs in ("x6", "x6h3", "w2x", "x6w1h"):
                t.w2x = pack()
            if packs in ("h3", "x6h3", "x6w1h"):
                t.w1h = pack()
            if packs in ("h3", "x6h3"):
                t.w2h = pack()
            t.t_end, t.rtol, t.atol, t.max_attempts = 0.5, 1e-5, 1e-6, kw.pop("max_attempts", 1000)
            t.steps = 6
        elif fn in TRAIN:
            t.t_end, t.steps = torch.empty(1), kw.pop("steps", 3)
            for k in ("w1h", "w2h") if "_h3" in fn else ("w1x", "w2x"):
                setattr(t, k, pack())
            if fn == "cnf_train_fwd":
                kw["e"] = True
        else:
            t.w1x, t.w2x, t.w1h, t.w2h = pack(), pack(), pack(), pack()
        if kw.pop("e", False):
            t.e, t.logp = torch.empty(BT, n, 3), torch.empty(BT, n, 1)
        if kw.pop("mbn", False):
            t.mbn_in, t.mbn_out = torch.empty(12), torch.empty(12)
        if kw.pop("table", False) or fn in FRAMES:
            t.steps = torch.empty(BT, dtype=torch.int32)
        if kw.pop("order", False):
            t.order = torch.empty(BT, dtype=torch.int32)
        if kw.pop("out", False):
            t.out = torch.empty(BT, n, 3)
        t.max_steps = kw.pop("max_steps", 4 if fn in FRAMES else None)
        if kw.pop("ys", False):
            t.ys, t.ka = torch.empty(t.max_steps, 4, BT, n, 3), torch.empty(t.max_steps, 4, BT, n, 3)
        if "bad" in kw:
            _violate(t, n, kw.pop("bad"), fn)
        no_grad, solve, reverse = kw.pop("no_grad", False), kw.pop("solve", False), kw.pop("reverse", False)
        kw.pop("capturing", None)
        w1, w2 = (t.w1h, t.w2h) if "_h3" in fn else (t.w1x, t.w2x)          # the packs of a training wrapper
        roles = {v.data_ptr(): k for k, v in vars(t).items() if isinstance(v, torch.Tensor) and v.device.type == "cpu"}
        mp.setattr(torch, "empty", keeping(torch.empty))
        mp.setattr(torch, "empty_like", keeping(torch.empty_like))
        try:
            if fn == "cnf_rk4":
                ret = ops.cnf_rk4(t.y, t.hyper, t.tcol, t.w0, t.b0, SimpleNamespace(data=t.w1p), t.b1, SimpleNamespace(data=t.w2p), t.b2, t.w3, t.b3,
                                  t.t_end, t.steps, reverse, mbn_in=t.mbn_in, mbn_out=t.mbn_out, e=t.e, logp=t.logp, w1x=t.w1x, w2x=t.w2x, w1h=t.w1h, w2h=t.w2h,
                                  order=t.order, max_steps=t.max_steps, out=t.out, **kw)
            elif fn == "cnf_dopri5":
                with torch.set_grad_enabled(not no_grad):
                    ret = ops.cnf_dopri5(t.y, t.hyper, t.tcol, t.w0, t.b0, t.b1, t.b2, t.w3, t.b3, t.w1x, t.w2x, t.t_end, t.rtol, t.atol, reverse,
                                         mbn_in=t.mbn_in, mbn_out=t.mbn_out, e=t.e, logp=t.logp, max_attempts=t.max_attempts, w1h=t.w1h, w2h=t.w2h, **kw)
            elif fn == "cnf_train_fwd":
                ret = train_ops.cnf_train_fwd(t.y, t.logp, t.e, t.hyper, t.tcol, t.w0, t.b0, w1, t.b1, w2, t.b2, t.w3, t.b3, t.t_end, t.steps, **kw)
            elif fn in FRAMES:
                ret = getattr(train_ops, fn)(t.y, t.hyper, t.tcol, t.w0, t.b0, w1, t.b1, w2, t.b2, t.w3, t.b3, t.t_end, t.steps, t.max_steps,
                                             order=t.order, ys=t.ys, ka=t.ka, **kw)
            elif fn in TRAIN:
                ret = getattr(train_ops, fn)(t.y, t.hyper, t.tcol, t.w0, t.b0, w1, t.b1, w2, t.b2, t.w3, t.b3, t.t_end, t.steps, **kw)
            else:
                P = flow_grad._SolvePacks
                ret = flow_grad._sample_tape_route(P(t.w1x, t.w1h) if solve else t.w1x, P(t.w2x, t.w2h) if solve else t.w2x, n, **kw)
        except Exception as e:        # noqa: BLE001 -- whatever it is, it is the transcript's last word
            log.append(["raise", type(e).__name__, str(e)])
        else:
            ret = ret if isinstance(ret, tuple) else (ret,)
            for i, r in enumerate(ret):
                if isinstance(r, torch.Tensor):
                    roles.setdefault(r.data_ptr(), "ret[%d]" % i)
            log.append(["return"] + [_returned(r) for r in ret])
        log.append(["end"] + list(ops.TIMERS))
    roles[None] = "null"
    roles[word.data_ptr()] = "word"
    if state.ws is not None:
        roles[state.ws.data_ptr()] = "ws"
    for v in state.new:
        roles.setdefault(v.data_ptr(), "new:%s:%s" % (str(v.dtype).replace("torch.", ""), "x".join(map(str, v.shape))))

    def named(v):
        if isinstance(v, tuple):
            return roles.get(v[1], "unknown")
        return [named(u) for u in v] if isinstance(v, list) else v
    return [named(line) for line in log]


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
