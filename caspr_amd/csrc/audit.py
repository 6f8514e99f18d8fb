"""Code-object audit of the kernels that manage the accumulator file by hand (ode_bf16x6w.hip, its f16x3 copy ode_f16x3w.hip, the adaptive solve ode_dp5_f16x3w.hip and the taped sampling solve ode_sample_tape_h3w.hip on the same evaluation text (ode_h3w_eval.inc), gemm_bf16x6w.hip, its f16x3 copy gemm_f16x3w.hip).

Both keep 256 live values at FIXED addresses a0..a255 across separate inline-asm statements.  A clobber list does not reserve
registers between statements: what keeps hipcc out of the AGPRs is the hidden flag -amdgpu-mfma-vgpr-form (build.py EXTRA) plus the
fact that a kernel without spills has no reason to park anything there.  Neither is a contract, so the BUILD checks the result:
build.build() runs audit_objects() on the objects it links and refuses to produce the library when the check trips (a silently
corrupted headline kernel is worse than no library).  tests/test_host_cpu.py runs the same functions on the in-tree objects.

TESTED_HIPCC is the compiler the committed expectations were measured with; another version is not an error in itself (the audit
decides), but the message of a failed audit names both."""
import os
import re
import subprocess
import tempfile

LLVM = os.environ.get("CASPR_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TESTED_HIPCC = "HIP version: 7.2.26015-fc0010cf6a / AMD clang version 22.0.0git roc-7.2.0"


class AuditError(RuntimeError):
    pass


def tools_present():
    return all(os.path.exists(os.path.join(LLVM, t)) for t in ("llvm-objdump", "llvm-objcopy", "llvm-readelf", "clang-offload-bundler"))


def _code_object(obj):
    """-> (notes text, disassembly text) of the gfx950 code object bundled in a hipcc -c object."""
    with tempfile.TemporaryDirectory() as d:
        fat, elf = os.path.join(d, "w.fatbin"), os.path.join(d, "w.elf")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj, os.path.join(d, "copy.o")])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + elf])
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], text=True)
        dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", elf], text=True)
    return notes, dis


def _kernel(notes, dis, name, whole=False):
    """-> (the metadata entry of kernel `name` in the amdhsa.kernels note, its instruction list).  The note is a YAML list whose
    entries start with "  - ." at list depth; the entry is found by its `.name:` line, not by character windows.  The instruction list
    ends at the kernel's first s_endpgm; with `whole` at its LAST one in front of the next symbol (a kernel whose early return the
    compiler gave an s_endpgm of its own in the prologue)."""
    entry, cur = None, []
    for ln in notes.splitlines() + ["  - .end"]:
        if re.match(r"^\s{0,4}- \.", ln):
            if any(re.match(r"^\s*(- )?\.name:\s+%s\s*$" % re.escape(name), l) for l in cur):
                entry = "\n".join(cur)
                break
            cur = [ln]
        else:
            cur.append(ln)
    if entry is None:
        raise AuditError("%s: no metadata entry in the code object's notes" % name)
    try:
        body = dis[dis.index("<%s>:" % name):]
        if whole:
            nxt = re.search(r"^[0-9a-f]+ <[^>]+>:$", body[1:], re.M)
            body = body[:nxt.start() + 1] if nxt else body
            body = body[:body.rindex("s_endpgm")]
        else:
            body = body[:body.index("s_endpgm")]
    except ValueError:
        raise AuditError("%s: not found in the disassembly" % name) from None
    ins = [ln.split("//")[0].strip() for ln in body.splitlines() if ln.startswith("\t")]
    return entry, ins


def _need(cond, what):
    if not cond:
        raise AuditError(what)


def _no_spills(meta, ins, k):
    _need(re.search(r"\.private_segment_fixed_size:\s+0\b", meta) and re.search(r"\.vgpr_spill_count:\s+0\b", meta), "%s: scratch / spills in the metadata" % k)
    _need(not any(i.startswith("scratch_") for i in ins), "%s: scratch instructions" % k)


def audit_cnf_x6w(obj):
    """cnf_rk4_x6w_kernel: no scratch, exactly the accumulator moves the source writes (256 zeroing writes + 256 in-place activation
    writes, 256 + 256 reads in pass 0 / passes 1-3), layer 1's MFMAs on a[..], every other MFMA in the VGPR form, M0 written once per
    LDS-DMA statement and by nothing else."""
    notes, dis = _code_object(obj)
    k = "_Z18cnf_rk4_x6w_kernel9CnfX6Args"
    meta, ins = _kernel(notes, dis, k)
    count = lambda pat: sum(1 for i in ins if re.match(pat, i))
    _no_spills(meta, ins, k)
    _need(re.search(r"\.agpr_count:\s+256\b", meta), k + ": agpr_count != 256")
    r, w = count(r"v_accvgpr_read_b32"), count(r"v_accvgpr_write_b32")
    _need(r == 512 and w == 512 and count(r"v_accvgpr_mov") == 0, "%s: %d reads / %d writes of the accumulator file (512 / 512 in the source): the compiler touches it" % (k, r, w))
    mfma = [i for i in ins if i.startswith("v_mfma")]
    on_acc = [i for i in mfma if re.match(r"v_mfma_f32_32x32x16_bf16 a\[", i)]
    _need(len(on_acc) == 8 * 4 * 12 and all(" a[" not in i for i in mfma if i not in on_acc), "%s: %d of %d MFMAs on a[..] (384 expected, all others on VGPRs)" % (k, len(on_acc), len(mfma)))
    dma = count(r"global_load_lds_dwordx4")
    m0 = sum(1 for i in ins if re.search(r"\bm0\b", i))
    _need(dma > 20 and m0 == dma - 10, "%s: %d LDS-DMA instructions, %d M0 accesses" % (k, dma, m0))
    return {"kernel": k, "accvgpr_reads": r, "accvgpr_writes": w, "mfma": len(mfma), "mfma_on_acc": len(on_acc), "lds_dma": dma}


def _m0_is_the_dmas(ins, k):
    """M0 belongs to the LDS-DMA statements: the only instructions that name it are their `s_mov_b32 m0, sN` (one per PIECE: the four
    loads of a wave's share differ by the instruction's immediate offset, which applies to the LDS side too), every such write has
    a load behind it before the next one, no load comes before the first write, and none sits directly behind a write (the wait
    state the load needs after an SALU write of M0).  -> the number of M0 writes."""
    last, writes = None, 0
    for n, i in enumerate(ins):
        if re.search(r"\bm0\b", i):
            _need(re.match(r"s_mov_b32 m0, s\d+$", i), "%s: M0 touched by `%s`" % (k, i))
            _need(last != "w", "%s: two M0 writes with no LDS-DMA instruction between them" % k)
            last, writes = "w", writes + 1
        elif i.startswith("global_load_lds_dwordx4"):
            _need(last is not None, "%s: an LDS-DMA instruction in front of the first M0 write" % k)
            _need(not ins[n - 1].startswith("s_mov_b32 m0"), "%s: an LDS-DMA instruction directly behind its M0 write" % k)
            last = "d"
    _need(writes > 0 and last == "d", "%s: %d M0 writes, the last one unused" % (k, writes))
    return writes


def audit_cnf_h3w(obj):
    """cnf_rk4_h3w_kernel (ode_f16x3w.hip, the f16x3 copy of the kernel above): no scratch, exactly the accumulator moves the source
    writes (256 zeroing writes + 256 plane writes; 256 reads in pass 0, 256 plane reads in passes 1-3), layer 1's MFMAs (8 pieces x 4
    regions x 6) on a[..] in the f16 form, every other MFMA in the VGPR form, M0 written by the LDS-DMA statements only (_m0_is_the_dmas).
    Also returned, not judged here: cvt_pk, the number of v_cvt_pk_f16_f32 (one per value pair and plane the kernel splits;
    tests/test_f16x3_planes_audit.py pins it)."""
    return _audit_h3w_rk4_loop(obj, "_Z18cnf_rk4_h3w_kernel9CnfH3Args")


def _audit_h3w_rk4_loop(obj, k, whole=False):
    """What audit_cnf_h3w asks, of kernel `k` of `obj`: a fixed-step RK4 loop around ONE copy of the f16x3 evaluation text in the
    instruction stream of cnf_rk4_h3w_kernel."""
    notes, dis = _code_object(obj)
    meta, ins = _kernel(notes, dis, k, whole)
    count = lambda pat: sum(1 for i in ins if re.match(pat, i))
    _no_spills(meta, ins, k)
    _need(re.search(r"\.agpr_count:\s+256\b", meta), k + ": agpr_count != 256")
    r, w = count(r"v_accvgpr_read_b32"), count(r"v_accvgpr_write_b32")
    _need(r == 512 and w == 512 and count(r"v_accvgpr_mov") == 0, "%s: %d reads / %d writes of the accumulator file (512 / 512 in the source): the compiler touches it" % (k, r, w))
    mfma = [i for i in ins if i.startswith("v_mfma")]
    on_acc = [i for i in mfma if re.match(r"v_mfma_f32_32x32x16_f16 a\[", i)]
    _need(len(on_acc) == 8 * 4 * 6 and all(" a[" not in i for i in mfma if i not in on_acc), "%s: %d of %d MFMAs on a[..] (192 expected, all others on VGPRs)" % (k, len(on_acc), len(mfma)))
    _need(all(i.startswith("v_mfma_f32_32x32x16_f16") for i in mfma), "%s: an MFMA that is not v_mfma_f32_32x32x16_f16" % k)
    dma = count(r"global_load_lds_dwordx4")
    m0 = _m0_is_the_dmas(ins, k)
    _need(dma > 20, "%s: %d LDS-DMA instructions" % (k, dma))
    vgpr = re.search(r"\.vgpr_count:\s+(\d+)", meta)
    return {"kernel": k, "accvgpr_reads": r, "accvgpr_writes": w, "mfma": len(mfma), "mfma_on_acc": len(on_acc), "lds_dma": dma, "m0_writes": m0,
            "cvt_pk": count(r"v_cvt_pk_f16_f32"), "vgpr_count": int(vgpr.group(1)) if vgpr else None}


def audit_cnf_sample_tape_h3w(obj):
    """cnf_sample_tape_h3w_kernel (ode_sample_tape_h3w.hip: cnf_rk4_h3w_kernel's loop around the same evaluation text, with the tape
    stores of the differentiable decode()): the contract of audit_cnf_h3w, count for count -- the tape stores are plain global stores
    and change none of them.  Its early return (a frame with a step count of 0) has an s_endpgm of its own: the whole body is read."""
    return _audit_h3w_rk4_loop(obj, "_Z26cnf_sample_tape_h3w_kernel19CnfSampleTapeH3Args", whole=True)


def audit_cnf_dp5_h3w(obj):
    """cnf_dp5_h3w_kernel (ode_dp5_f16x3w.hip: the adaptive Dormand-Prince loop around the evaluation of the kernel above, one text with it): the contract
    of audit_cnf_h3w -- no scratch, agpr_count 256, exactly the accumulator moves the source writes (the stage body ONCE in the code: 256
    zeroing writes + 256 plane writes; 256 reads in pass 0, 256 plane reads in passes 1-3) and no v_accvgpr_mov, layer 1's MFMAs (8
    pieces x 4 regions x 6) on a[..], every other MFMA in the VGPR form, all of them v_mfma_f32_32x32x16_f16, M0 touched by the LDS-DMA
    statements only.  Also returned, not judged: cvt_pk, and vgpr_count, the metadata's `.vgpr_count` -- on gfx950 the COMBINED register count of a wave, the
    VGPRs rounded up to the allocation granule of 8 plus the 256 accumulators (488 = 232 + 256 with the tested compiler, whose resource remark counts
    229 VGPRs in use; cnf_rk4_h3w_kernel: 464 = 208 + 256)."""
    notes, dis = _code_object(obj)
    k = "_Z18cnf_dp5_h3w_kernel12CnfDp5H3Args"
    meta, ins = _kernel(notes, dis, k)
    count = lambda pat: sum(1 for i in ins if re.match(pat, i))
    _no_spills(meta, ins, k)
    _need(re.search(r"\.agpr_count:\s+256\b", meta), k + ": agpr_count != 256")
    r, w = count(r"v_accvgpr_read_b32"), count(r"v_accvgpr_write_b32")
    _need(r == 512 and w == 512 and count(r"v_accvgpr_mov") == 0, "%s: %d reads / %d writes of the accumulator file (512 / 512 in the source): the compiler touches it" % (k, r, w))
    mfma = [i for i in ins if i.startswith("v_mfma")]
    on_acc = [i for i in mfma if re.match(r"v_mfma_f32_32x32x16_f16 a\[", i)]
    _need(len(on_acc) == 8 * 4 * 6 and all(" a[" not in i for i in mfma if i not in on_acc), "%s: %d of %d MFMAs on a[..] (192 expected, all others on VGPRs)" % (k, len(on_acc), len(mfma)))
    _need(all(i.startswith("v_mfma_f32_32x32x16_f16") for i in mfma), "%s: an MFMA that is not v_mfma_f32_32x32x16_f16" % k)
    dma = count(r"global_load_lds_dwordx4")
    m0 = sum(1 for i in ins if re.search(r"\bm0\b", i))
    _need(dma > 20 and m0 == dma, "%s: %d LDS-DMA instructions, %d M0 accesses" % (k, dma, m0))
    vgpr = re.search(r"\.vgpr_count:\s+(\d+)", meta)
    return {"kernel": k, "accvgpr_reads": r, "accvgpr_writes": w, "mfma": len(mfma), "mfma_on_acc": len(on_acc), "lds_dma": dma,
            "cvt_pk": count(r"v_cvt_pk_f16_f32"), "vgpr_count": int(vgpr.group(1)) if vgpr else None}


def audit_conv_x6w(obj):
    """conv1x1_x6w_kernel (all instantiations; persistent since round 4): no scratch, every MFMA on the hand-managed a[..] tiles, the
    accumulator file zeroed once in the prologue and read out + zeroed again in the two instances of the tile read-out (one per chunk
    parity): 3 x 256 writes, 2 x 256 reads, and nothing else."""
    notes, dis = _code_object(obj)
    kernels = re.findall(r"<(_Z18conv1x1_x6w_kernelI[^>]*)>:", dis)
    _need(len(kernels) >= 4, "conv1x1_x6w_kernel: %d instantiations found" % len(kernels))
    out = []
    for k in kernels:
        meta, ins = _kernel(notes, dis, k)
        count = lambda pat: sum(1 for i in ins if re.match(pat, i))
        _no_spills(meta, ins, k)
        r, w = count(r"v_accvgpr_read_b32"), count(r"v_accvgpr_write_b32")
        _need(w == 768 and r == 512 and count(r"v_accvgpr_mov") == 0, "%s: %d reads / %d writes of the accumulator file (512 / 768 in the source)" % (k, r, w))
        mfma = [i for i in ins if i.startswith("v_mfma")]
        _need(len(mfma) == 2 * 192 and all(re.match(r"v_mfma_f32_32x32x16_bf16 a\[", i) for i in mfma), "%s: %d MFMAs, not all on a[..]" % (k, len(mfma)))
        out.append({"kernel": k, "accvgpr_reads": r, "accvgpr_writes": w, "mfma": len(mfma)})
    return out


def audit_conv_h3w(obj):
    """conv1x1_h3w_kernel (gemm_f16x3w.hip, the f16x3 copy of the kernel above; all instantiations): no scratch, the accumulator file
    zeroed once in the prologue and read out + zeroed again in the two instances of the tile read-out (3 x 256 writes, 2 x 256 reads), two
    chunk bodies of 96 MFMAs, every one v_mfma_f32_32x32x16_f16 on a[..].  Also returned, not judged: cvt_pk, the number of
    v_cvt_pk_f16_f32 (one per value pair and plane the kernel splits)."""
    notes, dis = _code_object(obj)
    kernels = re.findall(r"<(_Z18conv1x1_h3w_kernelI[^>]*)>:", dis)
    _need(len(kernels) >= 4, "conv1x1_h3w_kernel: %d instantiations found" % len(kernels))
    out = []
    for k in kernels:
        meta, ins = _kernel(notes, dis, k)
        count = lambda pat: sum(1 for i in ins if re.match(pat, i))
        _no_spills(meta, ins, k)
        r, w = count(r"v_accvgpr_read_b32"), count(r"v_accvgpr_write_b32")
        _need(w == 768 and r == 512 and count(r"v_accvgpr_mov") == 0, "%s: %d reads / %d writes of the accumulator file (512 / 768 in the source)" % (k, r, w))
        mfma = [i for i in ins if i.startswith("v_mfma")]
        _need(len(mfma) == 2 * 96 and all(re.match(r"v_mfma_f32_32x32x16_f16 a\[", i) for i in mfma), "%s: %d MFMAs, not all v_mfma_f32_32x32x16_f16 on a[..]" % (k, len(mfma)))
        out.append({"kernel": k, "accvgpr_reads": r, "accvgpr_writes": w, "mfma": len(mfma), "cvt_pk": count(r"v_cvt_pk_f16_f32")})
    return out


AUDITS = {"ode_bf16x6w.hip": audit_cnf_x6w, "ode_f16x3w.hip": audit_cnf_h3w, "ode_dp5_f16x3w.hip": audit_cnf_dp5_h3w, "ode_sample_tape_h3w.hip": audit_cnf_sample_tape_h3w,
          "gemm_bf16x6w.hip": audit_conv_x6w, "gemm_f16x3w.hip": audit_conv_h3w}


def audit_objects(objs_by_source):
    """objs_by_source: {source file name: object path}.  Raises AuditError (naming the compiler) on the first violation -- including
    missing LLVM tools and anything unexpected while taking the code object apart.  CASPR_SKIP_AUDIT=1 (build.py) turns a failure
    into a loud warning: for a ROCm point release that schedules differently but correctly -- after `pytest -m gpu` has shown that
    the two kernels still compute what the oracle says."""
    if not tools_present():
        raise AuditError("the ROCm LLVM tools (%s: llvm-objdump, llvm-objcopy, llvm-readelf, clang-offload-bundler) are needed to audit the "
                         "hand-managed accumulator kernels" % LLVM)
    res = {}
    for src, fn in AUDITS.items():
        if src in objs_by_source:
            try:
                res[src] = fn(objs_by_source[src])
            except (AuditError, ValueError, IndexError, subprocess.CalledProcessError) as e:
                ver = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--version"], capture_output=True, text=True).stdout.splitlines()[:2]
                raise AuditError("%s\n  this compiler: %s\n  tested with:   %s\n  -> the library is NOT produced (CASPR_SKIP_AUDIT=1 overrides, "
                                 "see caspr_amd/csrc/audit.py)" % (e, " / ".join(ver), TESTED_HIPCC)) from None
    return res


def audit_no_packed_f32(objs_by_source):
    """No v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 in any product code object (build.py: NO_PACKED_F32).  Round 6: a packed-f32 operation that
    consumes a register an LDS read has just returned was seen to use the register's OLD content in one 16-lane pass when another kernel that also
    executes packed-f32 instructions shares the compute unit (tools/micro/pk_check.hip, profiles/r06_pk_check.txt); the library is built without the
    instruction class, and this check keeps a changed flag set or compiler from bringing it back unnoticed.  -> {source: 0}."""
    if not tools_present():
        raise AuditError("the ROCm LLVM tools (%s) are needed to check the objects for packed-f32 instructions" % LLVM)
    res = {}
    for src, obj in sorted(objs_by_source.items()):
        try:
            _, dis = _code_object(obj)
        except subprocess.CalledProcessError as e:
            raise AuditError("%s: could not take the code object apart (%s)" % (src, e)) from None
        hits = re.findall(r"\bv_pk_(?:add|mul|fma)_f32\b", dis)
        if hits:
            raise AuditError("%s: %d packed-f32 VALU instructions in the gfx950 code object (build.py compiles with -target-feature -packed-fp32-ops; see "
                             "audit_no_packed_f32)" % (src, len(hits)))
        res[src] = 0
    return res
