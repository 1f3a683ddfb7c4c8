#!/usr/bin/env python3
"""Instruction mix of the headline kernel's steady-state step, taken from the ISA the CURRENT sources compile to (gfx950): bench.py
reads the result (profiles/isa_mix.json) for its fp64-issue figures instead of hand-copied constants.

    python tools/isa_mix.py            # compiles xt_ll_r2_kernel<6,2,1> into /tmp, writes profiles/isa_mix.json

Method: the likelihood-only register-resident kernel (csrc/xt_reg2.h) unrolls its step loop over the F - 1 exchange phases in three
variants; the basic blocks with >= 40 fp64 vector instructions and the table reads are the steps.  The steady-state ones (well-scaled model:
zero-free, lazily re-normalised) are the 2 (F - 1) with the fewest instructions among the blocks of the innermost loops (the loop depth the
compiler notes at every block label); the first step-sized block outside them is the merge-free first step (position F - 1; the read-out of the last position follows it), and the warm-up chain (positions 1 .. F - 2)
is the one block with F - 2 v_rcp_f64 (the g-form launches' chain, which the headline runs), else the F - 2 blocks with one v_rcp_f64 right before the first step.  Counts are per wave-step (one wavefront = 64 / 2^(F-1) tracks,
one position).

The per-batch edge (once per wave-batch, outside the steps): the staging blocks are the blocks of the chunk loop (depth >= 2) from the first
one that loads 8 bytes from global memory up to the first block with a reciprocal (position 0 and the warm-up chains follow); the read-out is what follows the last step block up to the end of the
batch loop.  Both are STATIC counts over every block of the region - both sides of a branch, and the loop over partial batches next to the
path complete batches take - so they are upper bounds of what a wave executes; `staging_complete_batch_*` counts the blocks of the path that
a complete batch takes (the blocks with the scalar-base global loads and the ones they fall through to), when there is one.

    python tools/isa_mix.py --csrc DIR --no-write      # the same figures for another source tree (e.g. the parent's csrc), nothing written"""
import json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = sys.argv[sys.argv.index("--csrc") + 1] if "--csrc" in sys.argv else os.path.join(ROOT, "extrack_amd", "csrc")
F, D, K = 6, 2, 1
src = '''#include "xt_host.h"
#include "xt_reg2.h"
__global__ void __launch_bounds__(64 * XT_F2_WAVES) xt_ll_r2_kernel_mix(XtKernelArgs a)
{
    DevCtx cx;
    XtGradArgs ga;
    ga.dblob = nullptr;
    ga.gpartials = nullptr;
    xt_r2_body<%d, %d, %d, 0>(a, ga, cx);
}
''' % (F, D, K)
tmp = tempfile.mkdtemp(prefix="xt_isa_")
open(os.path.join(tmp, "mix.hip"), "w").write(src)
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.abspath(CSRC), "-c", "mix.hip",
                       "-o", "mix.o", "--save-temps"], cwd=tmp, stderr=subprocess.DEVNULL)
asm = [f for f in os.listdir(tmp) if f.endswith("gfx950.s")][0]
blocks, cur = [], None
for line in open(os.path.join(tmp, asm)):
    if line.startswith(".LBB") or line.startswith("_Z"):
        dm = re.search(r"Depth=(\d+)", line)
        cur = dict(name=line.split(":")[0], depth=int(dm.group(1)) if dm else 0, f64=0, fma=0, valu32=0, lds=0, salu=0, vmem=0, trans=0, xch=0, ld8=0, ld8s=0, vmwait=0)
        blocks.append(cur)
        continue
    if cur is not None and line.lstrip().startswith(";") and "Depth=" in line:  # the loop comment may follow the label on a line of its own
        cur["depth"] = int(re.search(r"Depth=(\d+)", line).group(1))
        continue
    if cur is None or not line.startswith("\t") or line.startswith("\t.") or line.startswith("\t;"):
        continue
    op = line.split()[0]
    if "permlane" in op or "_dpp" in op or " quad_perm:" in line or " row_" in line:
        cur["xch"] += 1  # an instruction of the lane exchange
    if op.startswith("v_"):
        if "_f64" in op or op in ("v_lshl_add_u64",):
            cur["f64"] += 1
            if "fma" in op or "fmac" in op:
                cur["fma"] += 1
            if op.startswith("v_rcp") or op.startswith("v_sqrt") or op.startswith("v_rsq"):
                cur["trans"] += 1
        else:
            cur["valu32"] += 1
    elif op.startswith("ds_"):
        cur["lds"] += 1
    elif op.startswith("s_"):
        cur["salu"] += 1
    elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        cur["vmem"] += 1
        if op in ("global_load_dwordx2", "flat_load_dwordx2"):
            cur["ld8"] += 1
            cur["ld8s"] += 1 if re.search(r", s\[\d+:\d+\]", line) else 0  # scalar base + one VGPR of offset
    if op == "s_waitcnt" and "vmcnt" in line:
        cur["vmwait"] += 1
steps = sorted([b for b in blocks if b["f64"] >= 40 and b["lds"] >= 4], key=lambda b: b["f64"] + b["valu32"])
maxd = max(b["depth"] for b in steps)
ss = [b for b in steps if b["depth"] == maxd][:2 * (F - 1)]  # the step loop is inlined twice (before / after the stay-in-FOV factor sets in): both copies of the F - 1 phases
# the merge-free first step: outside the innermost loops, one reciprocal, and - what tells it from the read-out of the last position - a lane
# exchange.  Both the general and the g-form first step are compiled; the headline runs the g-form one, the smaller of the two (the compiler
# may split it: its block with the exchange and the reciprocal is what is counted)
first = sorted([b for b in blocks if b["depth"] < maxd and b["trans"] == 1 and b["xch"] >= 8 and b["f64"] >= 20 and b["lds"] >= 4], key=lambda b: b["f64"])[:1]
at = blocks.index(first[0]) if len(first) == 1 else 0
chain = [b for b in blocks[:at] if b["depth"] == maxd - 1 and 10 <= b["f64"] < 40 and b["trans"] == 1][-(F - 2):] if at else []
# the g-form launches' chain (xt_r2_chain_g) has no exponential and compiles to ONE block for the full window: F - 2 reciprocals, no step's table pair
gchain = [b for b in blocks if b["depth"] == maxd - 1 and b["trans"] == F - 2 and b["f64"] < 40 * (F - 2)]
if len(gchain) == 1:
    chain = gchain
n = float(len(ss))
mix = {k: sum(b[k] for b in ss) / n for k in ("f64", "fma", "valu32", "lds", "salu", "vmem", "trans")}
tpw = 64 >> (F - 1)
out = {"kernel": "xt_ll_r2_kernel<%d,%d,%d> (steady-state step, mean over the %d exchange phases)" % (F, D, K, F - 1),
       "tracks_per_wave": tpw, "fp64_valu_per_wave_step": mix["f64"], "fp64_fma_per_wave_step": mix["fma"], "fp64_transcendental_per_wave_step": mix["trans"],
       "valu32_per_wave_step": mix["valu32"], "lds_per_wave_step": mix["lds"], "salu_per_wave_step": mix["salu"], "vmem_per_wave_step": mix["vmem"],
       "flop_per_wave_step": 64 * (mix["f64"] + mix["fma"]),
       "issue_cycles_per_wave_step": 4 * mix["f64"] + 2 * mix["valu32"],
       "method": "tools/isa_mix.py: hipcc --save-temps of the current csrc/xt_reg2.h; an fp64 vector instruction issues in 4 cycles per wavefront, "
                 "a 32-bit one (incl. the DPP moves of the lane exchange) in 2 (profiles/r01_valu_rates.txt); a v_permlane swap is counted as 32-bit",
       "step_blocks": [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in steps]}
# per-track fixed cost of the warm-up (once per wave-batch): the chain blocks together, the first full step
out["warmup_chain_blocks"] = [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in chain]
out["warmup_chain_fp64"] = sum(b["f64"] for b in chain)
out["warmup_chain_valu32"] = sum(b["valu32"] for b in chain)
out["warmup_chain_issue_cycles"] = 4 * out["warmup_chain_fp64"] + 2 * out["warmup_chain_valu32"]
out["first_step_blocks"] = [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in first]
out["first_step_fp64"] = sum(b["f64"] for b in first)
out["first_step_valu32"] = sum(b["valu32"] for b in first)
out["first_step_issue_cycles"] = 4 * out["first_step_fp64"] + 2 * out["first_step_valu32"]
# ---- the per-batch edge: staging before the warm-up chain, read-out after the last step block
def region(bs):
    return {"valu": sum(b["f64"] + b["valu32"] for b in bs), "lds": sum(b["lds"] for b in bs), "vmem": sum(b["vmem"] for b in bs),
            "vmcnt_waits": sum(b["vmwait"] for b in bs)}
ci = blocks.index(chain[0]) if chain else 0
st0 = next((i for i, b in enumerate(blocks[:ci]) if b["depth"] >= 2 and b["ld8"]), ci)  # depth 1 is the batch loop (and the loops of the prologue), 2 the chunk loop
ci = next((i for i in range(st0 + 1, ci) if blocks[i]["trans"]), ci)  # position 0 and the chains of the other step forms follow: the first reciprocal ends the staging
stage = [b for b in blocks[st0:ci] if b["depth"] >= 2]
fast = [i for i in range(st0, ci) if blocks[i]["ld8s"]]
fastb = []
if fast:  # from the first block with a scalar-base load to the next block that loads through a per-lane address (the loop over partial batches)
    end = next((i for i in range(fast[-1] + 1, ci) if blocks[i]["ld8"]), ci)
    fastb = [b for b in blocks[fast[0]:end] if b["f64"] + b["valu32"] + b["lds"] + b["vmem"] > 0 and "lr.ph" not in b["name"]]
last = max(i for i, b in enumerate(blocks) if b["depth"] == maxd)  # the last block of any step loop (all three step forms are compiled)
ro = []
for b in blocks[last + 1:]:
    if b["depth"] < 1:
        break
    ro.append(b)
for k, v in region(stage).items():
    out["staging_" + k] = v
for k, v in region(fastb).items():
    out["staging_complete_batch_" + k] = v
for k, v in region(ro).items():
    if k != "vmcnt_waits":
        out["readout_" + k] = v
out["staging_blocks"] = [(b["name"], b["f64"] + b["valu32"], b["lds"], b["vmem"], b["vmwait"]) for b in stage]
out["readout_blocks"] = [(b["name"], b["f64"] + b["valu32"], b["lds"], b["vmem"]) for b in ro]
# one wave-batch of L = 30 positions: 1 chain (positions 1 .. F - 2), the first step (F - 1), L - 1 - F steady steps, staging and read-out
LB = 30
stg = out["staging_complete_batch_valu"] or out["staging_valu"]
out["per_batch_valu_estimate"] = {"L": LB, "steady_steps": LB - 1 - F, "valu": round((LB - 1 - F) * (mix["f64"] + mix["valu32"]) + out["warmup_chain_fp64"] + out["warmup_chain_valu32"]
                                                                         + out["first_step_fp64"] + out["first_step_valu32"] + stg + out["readout_valu"], 1),
                                  "note": "to set against SQ_INSTS_VALU / wave-batches; the read-out and staging terms are static upper bounds"}
path = os.path.join(ROOT, "profiles", "isa_mix.json")
if "--no-write" not in sys.argv:
    json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if not k.endswith("_blocks")}, indent=1))
print("step blocks (name, fp64, 32-bit valu, lds):", out["step_blocks"])
