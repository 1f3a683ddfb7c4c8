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

    python tools/isa_mix.py --csrc DIR --no-write      # the same figures for another source tree (e.g. the parent's csrc), nothing written
    python tools/isa_mix.py --measured-cycles 10027    # modelled cycles per wave-batch beside a measured figure (busy cycles per wave-batch
                                                       # from the counters, profiles/readout_pmc_summary.txt): the residual is written down

Issue cycles per wave64 instruction (WEIGHTS): measured with tools/ubench/valu_rates.hip at 4 waves per SIMD, independent chains
(profiles/r01_valu_rates.txt, profiles/readout_valu_rates.txt), as multiples of the v_fma_f64 row of the same run (= 4 cycles).

The read-out is reported twice: `readout_*` is the static count over every block of the region (the old and the log-carried read-out, the
log() of the per-track output, the accumulation), `readout_executed_*` the path a g-form launch without per-track output takes (the
headline): the blocks from the one with the LDS atomic max of the log-carried read-out on, without the blocks of the per-track output
(from the branch on ll_out to the store), which are counted apart as `readout_per_track_output_*`."""
import json, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = sys.argv[sys.argv.index("--csrc") + 1] if "--csrc" in sys.argv else os.path.join(ROOT, "extrack_amd", "csrc")
F, D, K = 6, 2, 1
MEASURED = float(sys.argv[sys.argv.index("--measured-cycles") + 1]) if "--measured-cycles" in sys.argv else None
# cycles per wave64 instruction; classes in the order they are tested (weight_of)
# (nominal cycles of the row / 5.29, the mean of the warm and closing v_fma_f64 rows of profiles/readout_valu_rates.txt, x 4)
WEIGHTS = {"rcp_f64": 12.8,       # v_rcp_f64 alone, 16.95
           "f64": 4.0,            # fma / mul / add / ldexp (5.20) / min (4.81) / max / frexp / rndne
           "permlane_swap": 6.9,  # v_permlane16/32_swap_b32: 4.50 / 4.68 per exchanged dword, two per instruction
           "dpp": 3.4,            # v_mov_b32_dpp quad_perm 4.47, row_ror:8 4.45
           "cndmask": 2.0,        # (v_cmp_lt_u32 + v_cndmask_b32, 8.07) - (v_cmp_lt_u32 alone, 5.43) = 2.64; the bare row (23.6, a chain of
                                  # selects on a vcc that nothing writes) is not used
           "valu32_vop3": 3.7,    # three-operand 32-bit forms: v_bfe_u32 4.95, v_alignbit_b32 4.58, v_mad_u32 5.21
           "valu32": 2.2}         # two-operand 32-bit forms (_e32): v_add_u32 + v_xor_b32 5.76 per pair


def weight_of(op, line):
    if op.startswith("v_rcp_f64"):
        return "rcp_f64"
    if "_f64" in op or op == "v_lshl_add_u64":
        return "f64"
    if "permlane" in op:
        return "permlane_swap"
    if "_dpp" in op or " quad_perm:" in line or " row_" in line:
        return "dpp"
    if op.startswith("v_cndmask"):
        return "cndmask"
    return "valu32" if op.endswith("_e32") else "valu32_vop3"
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
def parse(fine):
    """Basic blocks of the kernel by label; fine: fall-through blocks (; %bb.N) apart as well."""
    blocks, cur = [], None
    for line in open(os.path.join(tmp, asm)):
        if fine and cur is not None and line.startswith("; %bb."):  # a fall-through block: no label of its own, same loop as the block before it
            cur = dict({k: 0 for k in cur}, name=cur["name"].split("+")[0] + "+" + line.split()[1].rstrip(":"), depth=cur["depth"], cyc=0.0)
            blocks.append(cur)
            continue
        if line.startswith(".LBB") or line.startswith("_Z"):
            dm = re.search(r"Depth=(\d+)", line)
            cur = dict(name=line.split(":")[0], depth=int(dm.group(1)) if dm else 0, f64=0, fma=0, valu32=0, lds=0, salu=0, vmem=0, trans=0, xch=0, ld8=0, ld8s=0, vmwait=0, cyc=0.0, dsmax=0, gst=0)
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
            cur["cyc"] += WEIGHTS[weight_of(op, line)]
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
            cur["dsmax"] += 1 if op.startswith("ds_max") else 0
        elif op.startswith("s_"):
            cur["salu"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            cur["vmem"] += 1
            cur["gst"] += 1 if op.startswith(("global_store", "flat_store")) else 0
            if op in ("global_load_dwordx2", "flat_load_dwordx2"):
                cur["ld8"] += 1
                cur["ld8s"] += 1 if re.search(r", s\[\d+:\d+\]", line) else 0  # scalar base + one VGPR of offset
        if op == "s_waitcnt" and "vmcnt" in line:
            cur["vmwait"] += 1
    return blocks


blocks = parse(False)
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
       "issue_cycles_per_wave_step": round(sum(b["cyc"] for b in ss) / n, 1),
       "issue_cycle_weights": WEIGHTS,
       "method": "tools/isa_mix.py: hipcc --save-temps of the current csrc/xt_reg2.h; cycles per wave64 instruction as measured by "
                 "tools/ubench/valu_rates.hip (profiles/r01_valu_rates.txt, profiles/readout_valu_rates.txt): issue_cycle_weights",
       "step_blocks": [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in steps]}
# per-track fixed cost of the warm-up (once per wave-batch): the chain blocks together, the first full step
out["warmup_chain_blocks"] = [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in chain]
out["warmup_chain_fp64"] = sum(b["f64"] for b in chain)
out["warmup_chain_valu32"] = sum(b["valu32"] for b in chain)
out["warmup_chain_issue_cycles"] = round(sum(b["cyc"] for b in chain), 1)
out["first_step_blocks"] = [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in first]
out["first_step_fp64"] = sum(b["f64"] for b in first)
out["first_step_valu32"] = sum(b["valu32"] for b in first)
out["first_step_issue_cycles"] = round(sum(b["cyc"] for b in first), 1)
# ---- the per-batch edge: staging before the warm-up chain, read-out after the last step block
def region(bs):
    return {"valu": sum(b["f64"] + b["valu32"] for b in bs), "fp64": sum(b["f64"] for b in bs), "lds": sum(b["lds"] for b in bs),
            "vmem": sum(b["vmem"] for b in bs), "vmcnt_waits": sum(b["vmwait"] for b in bs), "issue_cycles": round(sum(b["cyc"] for b in bs), 1)}
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
# the same region with the fall-through blocks apart: what tells the executed path from the branches around it
fineb = parse(True)
f0 = max(i for i, b in enumerate(fineb) if b["name"].split("+")[0] == blocks[last]["name"]) + 1
rof = []
for b in fineb[f0:]:
    if b["depth"] < 1:
        break
    rof.append(b)
for k, v in region(stage).items():
    out["staging_" + k] = v
for k, v in region(fastb).items():
    out["staging_complete_batch_" + k] = v
for k, v in region(ro).items():
    if k != "vmcnt_waits":
        out["readout_" + k] = v
# the executed read-out of a g-form launch without per-track output.  The per-track output is the block with the region's store (log() is
# inlined in front of it).  With the log-carried read-out (the block with the region's one LDS atomic max) the blocks between it and the lane
# sum (the last block with the DPP moves of xt_r2_gsum before the store) are the old read-out, which such a launch skips; without it (the
# parent) everything but the per-track output is executed.  The per-slot accumulation after the store sits at the head of the batch loop in
# the compiler's layout and is in neither figure, in either build.
dsm = [i for i, b in enumerate(rof) if b["dsmax"]]
gsts = [i for i, b in enumerate(rof) if b["gst"]]
if len(dsm) > 1 or len(gsts) != 1:
    sys.exit("tools/isa_mix.py: the read-out region has %d blocks with an LDS atomic max (0 or 1 expected) and %d with a store (1 expected): "
             "the compiler's layout changed, the executed read-out cannot be told apart" % (len(dsm), len(gsts)))
ro0, gst = (dsm[0] if dsm else None), gsts[0]
gss = [i for i, b in enumerate(rof[:gst]) if b["xch"] >= 8]
if not gss or (ro0 is not None and not ro0 < gss[-1]):
    sys.exit("tools/isa_mix.py: no lane sum (a block with >= 8 lane-exchange instructions) between the log-carried read-out and the store")
gs = gss[-1]
pto = rof[gst:gst + 1]
exe = [b for i, b in enumerate(rof) if i != gst and (ro0 is None or i == ro0 or i >= gs)]
print("executed read-out: anchors " + ", ".join("%s = %s" % (k, rof[i]["name"]) for k, i in (("atomic max", ro0), ("lane sum", gs), ("store", gst)) if i is not None)
      + "; counted blocks: " + " ".join(b["name"] for b in exe if b["f64"] + b["valu32"]), file=sys.stderr)
for k, v in region(exe).items():
    if k != "vmcnt_waits":
        out["readout_executed_" + k] = v
for k, v in region(pto).items():
    if k != "vmcnt_waits":
        out["readout_per_track_output_" + k] = v
out["readout_log_carried"] = ro0 is not None
out["readout_executed_blocks"] = [(b["name"], b["f64"], b["valu32"], b["lds"]) for b in exe]
out["staging_blocks"] = [(b["name"], b["f64"] + b["valu32"], b["lds"], b["vmem"], b["vmwait"]) for b in stage]
out["readout_blocks"] = [(b["name"], b["f64"] + b["valu32"], b["lds"], b["vmem"]) for b in ro]
# one wave-batch of L = 30 positions: 1 chain (positions 1 .. F - 2), the first step (F - 1), L - 1 - F steady steps, staging and read-out
LB = 30
stg = out["staging_complete_batch_valu"] or out["staging_valu"]
out["per_batch_valu_estimate"] = {"L": LB, "steady_steps": LB - 1 - F, "valu": round((LB - 1 - F) * (mix["f64"] + mix["valu32"]) + out["warmup_chain_fp64"] + out["warmup_chain_valu32"]
                                                                         + out["first_step_fp64"] + out["first_step_valu32"] + stg + out["readout_valu"], 1),
                                  "note": "to set against SQ_INSTS_VALU / wave-batches; the read-out and staging terms are static upper bounds"}
stgc = out["staging_complete_batch_issue_cycles"] if out["staging_complete_batch_valu"] else out["staging_issue_cycles"]
model = (LB - 1 - F) * out["issue_cycles_per_wave_step"] + out["warmup_chain_issue_cycles"] + out["first_step_issue_cycles"] + stgc + out["readout_executed_issue_cycles"]
out["per_batch_cycle_model"] = {"L": LB, "modelled_cycles": round(model, 1),
                                "valu_executed_estimate": round((LB - 1 - F) * (mix["f64"] + mix["valu32"]) + out["warmup_chain_fp64"] + out["warmup_chain_valu32"]
                                                                + out["first_step_fp64"] + out["first_step_valu32"] + stg + out["readout_executed_valu"], 1),
                                "note": "steady steps + chain + first step + staging of a complete batch + executed read-out; position 0 and the scalar "
                                        "bookkeeping between the blocks are not in it"}
if MEASURED is not None:
    out["per_batch_cycle_model"]["measured_cycles"] = MEASURED
    out["per_batch_cycle_model"]["residual_cycles"] = round(MEASURED - model, 1)
    out["per_batch_cycle_model"]["residual_fraction"] = round((MEASURED - model) / MEASURED, 4)
path = os.path.join(ROOT, "profiles", "isa_mix.json")
if "--no-write" not in sys.argv:
    json.dump(out, open(path, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if not k.endswith("_blocks")}, indent=1))
print("step blocks (name, fp64, 32-bit valu, lds):", out["step_blocks"])
