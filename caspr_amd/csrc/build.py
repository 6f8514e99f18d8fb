"""Build libcaspr_hip.so for gfx950 with hipcc (in-tree; the .so travels to the GPU box)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
SOURCES = ["point_ops.hip", "gemm.hip", "gemm_bf16x6.hip", "gemm_bf16x6w.hip", "gemm_f16x3w.hip", "sa_mlp.hip", "ode.hip", "ode_bf16x6.hip", "ode_bf16x6w.hip", "ode_f16x3w.hip", "cnf_frame_steps.hip", "ode_dp5.hip", "ode_dp5_f16x3w.hip", "ode_train_fwd.hip", "ode_sample_tape.hip", "ode_sample_tape_h3w.hip", "ode_latent_dp5.hip", "backward.hip", "backward_points.hip", "backward_flow.hip", "backward_flow_value.hip", "emd.hip", "emd_exact.hip", "pose.hip", "base_sample.hip"]
EXTRA = {"point_ops.hip": ["-ffp-contract=off"], "emd.hip": ["-ffp-contract=off"], "pose.hip": ["-ffp-contract=off"],
         "emd_exact.hip": ["-ffp-contract=off"],   # its f32 costs and f64 bids are restated operation by operation (tests/emd_exact_ref.py)
         "cnf_frame_steps.hip": ["-ffp-contract=off"],   # its f64 decisions are restated operation by operation (tests/frame_steps_ref.py)
         "base_sample.hip": ["-ffp-contract=off"],   # its log-density must round as ATen's separate kernels do (see the file's header)
         # the 64-piece product loop of the 64-point bf16x6 CNF evaluation (ode_x6_eval.inc, included by these four) must unroll
         # completely (static register indices)
         "ode_bf16x6.hip": ["-mllvm", "-pragma-unroll-threshold=400000"],
         "ode_dp5.hip": ["-mllvm", "-pragma-unroll-threshold=400000"],
         "ode_train_fwd.hip": ["-mllvm", "-pragma-unroll-threshold=400000"],
         "ode_sample_tape.hip": ["-mllvm", "-pragma-unroll-threshold=400000"],
         # the 128-point CNF kernel keeps its layer-1 accumulators in the accumulator file BY HAND (inline asm): hipcc's own MFMAs
         # must take the VGPR form there, or it would park them in AGPRs it believes free (see the kernel's header)
         "ode_bf16x6w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
         "ode_f16x3w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],   # the same, on f16 (ode_h3w_eval.inc)
         "ode_dp5_f16x3w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],   # ... the same text under the adaptive loop
         "ode_sample_tape_h3w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],   # ... and under the RK4 loop that writes the tape
         "gemm_bf16x6w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"],
         "gemm_f16x3w.hip": ["-mllvm", "-pragma-unroll-threshold=400000", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"]}   # its f16x3 copy
# CASPR_BUILD_DEBUG=1: the flavour with phase-trace hooks and experiment switches (-DCASPR_DEBUG_HOOKS, see common.h), built
# next to the production library as libcaspr_hip_debug.so with its own objects; tools/*_phase_trace.py load it.
DEBUG = os.environ.get("CASPR_BUILD_DEBUG", "0") not in ("0", "")
# CASPR_XW_EXP=<bits>: a debug flavour whose 128-point CNF kernel is compiled with -DXW_EXP=<bits> (timing experiments that
# switch parts of the kernel off at compile time, see ode_bf16x6w.hip; ode_f16x3w.hip has its own bits, which bring back the parent's
# instruction stream item by item) -> libcaspr_hip_debug_xw<bits>.so, for tools/cnf_x6w_trace.py --lib and tools/cnf_h3w_trace.py --lib
XW_EXP = os.environ.get("CASPR_XW_EXP", "")
DEBUG = DEBUG or bool(XW_EXP)
OUT = os.path.join(HERE, ("libcaspr_hip_debug_xw%s.so" % XW_EXP) if XW_EXP else ("libcaspr_hip_debug.so" if DEBUG else "libcaspr_hip.so"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# NO PACKED f32 VALU INSTRUCTIONS in this library (round 6): v_pk_add / v_pk_mul / v_pk_fma_f32 that consume a register an LDS read has just returned
# were seen to use the register's OLD content in one 16-lane pass when another kernel that also executes packed-f32 instructions shares the compute
# unit (tools/micro/pk_check.hip, profiles/r06_pk_check.txt: farthest-point sampling chose wrong centres beside the encoder's conv; it takes two).  The compiler had placed ~9,000 of them
# in these kernels on its own (SLP vectorisation, float2 / float4 arithmetic); without them the headline step is as fast (69.0 -> 68.85 ms).  The feature
# switch is a device feature: the host pass of hipcc prints a "not a recognized feature" note for it, filtered below; audit.py checks the objects.
NO_PACKED_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"] + NO_PACKED_F32


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def deps():
    """What every object depends on besides its source: this file (the flag set lives here), every header and every text fragment of
    this directory, the public headers.  Listed from the directories: a fragment that is missing here leaves a stale object behind."""
    inc = os.path.join(HERE, "..", "..", "include")
    return [os.path.abspath(__file__)] + sorted(os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith((".h", ".inc"))) + sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h"))


def build(force=False, verbose=False):
    hdrs = deps()
    objs, jobs, by_src = [], [], {}
    for s in SOURCES:
        src = os.path.join(HERE, s)
        xw = XW_EXP if (XW_EXP and s in ("ode_bf16x6w.hip", "ode_f16x3w.hip", "gemm_bf16x6w.hip", "gemm_f16x3w.hip")) else ""
        obj = os.path.join(HERE, s.replace(".hip", (".dbg_xw%s.o" % xw) if xw else (".dbg.o" if DEBUG else ".o")))
        objs.append(obj)
        if not xw:
            by_src[s] = obj
        if force or _stale(obj, [src] + hdrs):
            jobs.append([HIPCC] + FLAGS + (["-DCASPR_DEBUG_HOOKS"] if DEBUG else []) + (["-DXW_EXP=%s" % xw] if xw else []) + EXTRA.get(s, []) + ["-c", src, "-o", obj])
    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
        err = "\n".join(l for l in r.stderr.splitlines() if "'-packed-fp32-ops' is not a recognized feature for this target" not in l)
        if err.strip():
            sys.stderr.write(err + "\n")
        if r.returncode != 0:
            raise subprocess.CalledProcessError(r.returncode, cmd)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(OUT, objs):
        # the two kernels with a hand-managed accumulator file are checked on the code object BEFORE linking: a compiler that parks
        # values in a0..a255 or spills there would corrupt them silently (audit.py); the debug / experiment flavours carry trace hooks and switches that change the counts
        if not DEBUG:
            from caspr_amd.csrc import audit
            try:
                audit.audit_objects(by_src)
                audit.audit_no_packed_f32(by_src)
            except audit.AuditError as e:
                # CASPR_SKIP_AUDIT=1: link anyway (a ROCm point release that schedules or unrolls differently but correctly would
                # otherwise make the whole framework unbuildable); the GPU suite then is the judge of the two kernels
                if os.environ.get("CASPR_SKIP_AUDIT", "0") != "1":
                    raise
                import warnings
                warnings.warn("caspr_amd build: code-object audit FAILED and was skipped on request (CASPR_SKIP_AUDIT=1):\n%s\n"
                              "run `pytest -m gpu` before trusting cnf_rk4_x6w_kernel / cnf_rk4_h3w_kernel / cnf_dp5_h3w_kernel / cnf_sample_tape_h3w_kernel / conv1x1_x6w_kernel / conv1x1_h3w_kernel" % e, RuntimeWarning)
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
