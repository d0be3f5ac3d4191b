"""Instruction-level account of solve_packed_kernel: compiles lfr_solve.hip with -DLFR_ISA_MARKS (comment marks at the
phase boundaries, no GPU needed), walks the ISA of the kernel in textual order and counts the instructions of every phase by kind, per
packed class.  The counts are STATIC (one pass over the unrolled code: every edge slot, every elimination step, every instantiation of
the elimination once); next to the s_memtime phase profile (-DLFR_PROFILE_PHASES) they say what a phase's cycles are spent on.
Every class gets a second table, "VALU by family": its vector-ALU instructions again, per phase, split into fp64 arithmetic, conversions,
int32, plain v_mov, DPP moves, v_cndmask, v_cmp, lane moves (v_readlane / v_writelane / v_readfirstlane), v_accvgpr and the rest (listed
by mnemonic under the table); `non_arith` is everything but the first two.  Blocks are attributed in TEXTUAL order and the compiler lays
them out in its own: a class sum is reliable, a phase row approximate.
usage: python scripts/isa_account.py [kernel-substring [existing.s]] > profiles/r04_isa_account_packed_kernel.txt
(an existing ISA file given as the second argument is read instead of compiling; the default substring meets the warm-start
instantiation first: solve_packed_kernelILb0ELb0E names the cold record-reading kernel the bench runs).  The first line of the output
carries the kernel's VGPR count, scratch size and occupancy from the compiler's own comment block."""
import collections, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = os.path.join(ROOT, "local-feature-refinement_amd", "csrc")
want = sys.argv[1] if len(sys.argv) > 1 else "solve_packed_kernelILb0E"
out = "/tmp/lfr_solve_isa.s"
if len(sys.argv) > 2: out = sys.argv[2]
else: subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-DLFR_ISA_MARKS", "-I", os.path.join(ROOT, "include"), "-I", C,
                       "-S", "--cuda-device-only", os.path.join(C, "lfr_solve.hip"), "-o", out], stderr=subprocess.DEVNULL)
lines = open(out).read().split("\n")
start = [i for i, l in enumerate(lines) if re.match(r"^_Z\w*%s\w*:" % re.escape(want), l)][0]
# the kernel has one s_endpgm per exit and the compiler lays blocks out in its own order (<16,1,6> sits behind the first exit): the
# function ends at its .Lfunc_end label, not at the first s_endpgm
end = [i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end")][0]


def kind(op):
    if op.startswith("ds_add") or op.startswith("ds_pk_add") or op.startswith("ds_sub") or op.startswith("ds_max") or op.startswith("ds_min"): return "lds_atomic"
    if op.startswith("ds_swizzle") or op.startswith("ds_bpermute") or op.startswith("ds_permute"): return "lds_xbar"
    if op.startswith("ds_"): return "lds"
    if op.startswith("v_mfma"): return "mfma"
    if re.match(r"v_(fma|fmac|mul|add|max|min|rcp|rsq|sqrt|cmp\w*|cvt_f64|div|ldexp|frexp|trunc|floor|rndne|fract)_?\w*f64", op) or op.endswith("_f64") or "f64" in op: return "valu_f64"
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane"): return "lane"
    if op.startswith("v_"): return "valu_other"
    if op.startswith("ds_add") or op.startswith("ds_pk_add") or "ds_add" in op: return "lds_atomic"
    if op.startswith("ds_swizzle") or op.startswith("ds_bpermute") or op.startswith("ds_permute"): return "lds_xbar"
    if op.startswith("ds_"): return "lds"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith("s_cbranch") or op.startswith("s_branch"): return "branch"
    if op.startswith("s_load") or op.startswith("s_buffer"): return "smem"
    if op.startswith("s_"): return "salu"
    if op.startswith("global_") or op.startswith("buffer_") or op.startswith("flat_"): return "vmem"
    if op.startswith("scratch_"): return "scratch"
    return "other"


VALU_KINDS = ["f64_arith", "convert", "int32", "mov", "dpp_mov", "cndmask", "cmp", "lane", "accvgpr", "else"]
INT32 = re.compile(r"v_(add|sub|subrev|addc|subb|subbrev|mul_lo|mul_hi|mul_u32|mul_i32|mad|lshl|lshr|ashr|lshlrev|lshrrev|ashrrev|and|or|xor|xnor|not|bfe|bfi|bfm|alignbit|alignbyte|perm|"
                   r"min|max|med3|min3|max3|add3|lshl_add|lshl_or|add_lshl|and_or|or3|xad|mbcnt|bcnt|ffbh|ffbl|sad)\w*_(u32|i32|b32|u24|i24|u16|i16|b16|u64|i64|b64|u32_u24|i32_i24|lo_u32_b32|hi_u32_b32)(_e32|_e64|_sdwa)?$")


def valu_kind(op, text):
    """The split of the VALU row (the old table's valu_f64 + valu_other + lane): by mnemonic family alone.  A DPP operand on an fp64 instruction
    (the elimination's v_fmac_f64 row_newbcast) leaves it arithmetic; dpp_mov is a v_mov that exists to move a value across lanes."""
    is_dpp = "dpp" in op or "row_" in text or "quad_perm" in text or "wave_" in text
    if op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane"): return "lane"
    if op.startswith("v_accvgpr"): return "accvgpr"
    if op.startswith("v_cmp"): return "cmp"
    if op.startswith("v_cndmask"): return "cndmask"
    if op.startswith("v_cvt"): return "convert"
    if op.startswith("v_mov_b"): return "dpp_mov" if is_dpp else "mov"
    if "f64" in op: return "f64_arith"
    if INT32.match(op): return "int32"
    return "else"


NAMES = {"0": "prologue: edges -> registers", "loop_top": "iteration entry: convergence tests, LM diagonal, rows of A -> registers (all instantiations)", "1": "LM step tail (model change, transitions of A)", "5": "step setup: diagonal, build rows of A in registers",
         "gauss_jordan": "Gauss-Jordan elimination (all instantiations)", "step_reductions": "step: reductions, validity, trial point",
         "6": "zero J^T J in LDS", "sweep_setup": "sweep: slot setup", "eval": "sweep: edge evaluation (cost.cc model: interpolant, loss, corrector)",
         "assemble": "sweep: assembly (pair exchange through DPP, LDS atomics)", "eval_cost_only": "cost-only sweep: evaluation", "cost_only_loop": "cost-only sweep: loop",
         "2": "after the sweep: LDS sync", "3": "post-sweep reductions", "4": "transitions (convergence tests, line search bookkeeping)", "entry": "kernel entry / class dispatch"}
cls, mark = "entry", "entry"
acc = collections.defaultdict(lambda: collections.Counter())
vacc = collections.defaultdict(lambda: collections.Counter())          # the VALU row split by family
velse = collections.defaultdict(lambda: collections.Counter())         # what the split's last column holds, by mnemonic
dpp = collections.Counter()
for l in lines[start:end]:
    t = l.strip()
    m = re.match(r";\s*LFR_CLASS (\d+) (\d+) (\d+)", t)
    if m:
        cls = "<%s,%s,%s>" % m.groups(); mark = "0"; continue
    m = re.match(r";\s*LFR_MARK (\w+)", t)
    if m:
        mark = m.group(1); continue
    if not t or t[0] in ";." or t.endswith(":"): continue
    op = t.split()[0]
    acc[(cls, mark)][kind(op)] += 1
    if op.startswith("v_") and kind(op) != "mfma":
        vk = valu_kind(op, t)
        vacc[(cls, mark)][vk] += 1
        if vk == "else": velse[cls][re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)] += 1
    if "dpp" in op or "row_" in t or "quad_perm" in t: dpp[(cls, mark)] += 1
kinds = ["valu_f64", "valu_other", "lane", "lds", "lds_atomic", "lds_xbar", "vmem", "scratch", "smem", "salu", "waitcnt", "branch", "other"]
print("solve_packed_kernel<false>: static instruction counts per phase (compile-time unrolled code, one pass), from the ISA of this tree\n")
# the kernel's resources, from the comment block the compiler writes behind the function (one kernel holds every class: one register
# allocation; the scratch instructions of each class are the `scratch` column below)
res = {}
for l in lines[end:end + 80]:
    m = re.match(r";\s*(NumVgprs|NumAgprs|NumSgprs|ScratchSize|Occupancy|codeLenInByte)\s*[:=]\s*(\d+)", l)
    if m and m.group(1) not in res: res[m.group(1)] = int(m.group(2))
print("kernel %s: %s\n" % (lines[start].split(":")[0], "  ".join("%s %d" % kv for kv in res.items())))
order = ["0", "loop_top", "5", "gauss_jordan", "step_reductions", "1", "6", "sweep_setup", "eval", "assemble", "eval_cost_only", "cost_only_loop", "2", "3", "4"]
for c in sorted({k[0] for k in acc}):
    print("class %s" % c)
    print("  %-62s %6s | %s | dpp" % ("phase", "total", " ".join("%9s" % k[:9] for k in kinds)))
    tot = collections.Counter()
    for mk in order + sorted({k[1] for k in acc if k[0] == c} - set(order)):
        a = acc.get((c, mk))
        if not a: continue
        n = sum(a.values())
        tot.update(a)
        print("  %-62s %6d | %s | %4d" % (NAMES.get(mk, mk)[:62], n, " ".join("%9d" % a[k] for k in kinds), dpp[(c, mk)]))
    print("  %-62s %6d | %s" % ("sum", sum(tot.values()), " ".join("%9d" % tot[k] for k in kinds)))
    # the VALU instructions of the class again (valu_f64 + valu_other + lane above), split by family: what is arithmetic and what only
    # moves, selects and compares.  non_arith = everything but f64_arith and convert
    print("  %-62s %6s | %s | non_arith" % ("VALU by family", "valu", " ".join("%9s" % k[:9] for k in VALU_KINDS)))
    vtot = collections.Counter()
    for mk in order + sorted({k[1] for k in vacc if k[0] == c} - set(order)):
        a = vacc.get((c, mk))
        if not a: continue
        vtot.update(a)
        print("  %-62s %6d | %s | %6d" % (NAMES.get(mk, mk)[:62], sum(a.values()), " ".join("%9d" % a[k] for k in VALU_KINDS), sum(a.values()) - a["f64_arith"] - a["convert"]))
    print("  %-62s %6d | %s | %6d" % ("sum", sum(vtot.values()), " ".join("%9d" % vtot[k] for k in VALU_KINDS), sum(vtot.values()) - vtot["f64_arith"] - vtot["convert"]))
    print("  else: " + "  ".join("%s %d" % kv for kv in velse[c].most_common()))
    print()
