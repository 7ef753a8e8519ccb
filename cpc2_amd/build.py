"""Builds libcpc2_hip.so (gfx950) in-tree with hipcc.  `python -m cpc2_amd.build`."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcpc2_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ["gemm_f32.hip", "gemm_planes.hip", "rowops.hip", "encoder.hip", "gru.hip", "lstm.hip", "infonce.hip", "side_stream.hip", "transformer.hip", "abx.hip", "abx_units.hip", "sdtw.hip", "lalign.hip", "sdtw_units.hip", "lalign_units.hip", "kmeans.hip", "moments.hip", "seqmoments.hip", "mfcc.hip", "probe.hip", "augment.hip", "pitch.hip", "freeverb.hip", "bandreject.hip", "resample.hip", "text.hip", "seqalign.hip", "ctc_head.hip", "ctc_align.hip", "segment.hip", "unit_scores.hip", "unit_dp.hip", "negidx.cpp", "flac.cpp"]
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-pthread"]
# Device code is built WITHOUT the packed-f32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32).  Round 3 found
# (profiles/r03_dp_rootcause.md; tools/load_determinism_probe.py reproduces it) that kernels which hipcc
# had packed -- conv0_bwd_kernel first of all -- returned slightly different sums from one launch to the next, on the same
# inputs in the same registers, whenever ANOTHER process ran short kernels on the same MI355X: 10-39 % of launches with the
# instructions, 0 of 1 260 without, at no measurable cost (5.42 against 5.43-5.64 ms per step; the guide lists packed f32
# beside MFMAs as an anti-lever anyway).  The host pass does not know the feature and says so: that line is filtered.
DEVICE_FLAGS = ["--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
# seqalign.hip restates a float32 numpy program operation for operation: a product and the sum behind it must stay two roundings.
# hipcc's default (-ffp-contract=fast) fuses them whatever the source says (__fmul_rn / __fadd_rn are plain operators, a pragma
# is not honoured), so contraction is off for that file.  ctc_align.hip states its recurrence as a max followed by ONE f64 addition
# that a host program repeats bit for bit: the same flag keeps any later product in that file from being fused into it.
# pitch.hip states a candidate's cost as a difference, its square and one f64 addition per term, and the segment starts it picks
# must EQUAL those of a numpy program: a square fused into the addition would move near-ties.
# segment.hip keeps a peak when prom >= p * range, and the kept peaks must EQUAL those of a numpy program: the product is one
# rounding of its own, never fused into what surrounds it.
# freeverb.hip states every sample as the float32 operations of its definition, in their order (s = o + (s - o) dmp is a
# difference, a product and a sum): unfused, its output equals a float32 numpy evaluation of the definition.
# unit_dp.hip states its recurrence as a comparison and ONE f64 addition per state and frame, which a numpy program repeats bit
# for bit: the flag keeps any later product in that file from being fused into them.
# lalign.hip states a cell as one f32 subtraction per candidate and one f32 addition, and its scores and spans must EQUAL those of a
# float32 numpy program: the flag keeps any later product in that file from being fused into them (the distance tile of
# dist_tile.h spells its fma chain out, so it is the same under either setting).  lalign_units.hip runs the same recurrence
# (lalign_rule.h) on unit ids under the same flag.
FILE_FLAGS = {"seqalign.hip": ["-ffp-contract=off"], "ctc_align.hip": ["-ffp-contract=off"], "pitch.hip": ["-ffp-contract=off"],
              "segment.hip": ["-ffp-contract=off"], "freeverb.hip": ["-ffp-contract=off"], "unit_dp.hip": ["-ffp-contract=off"],
              "lalign.hip": ["-ffp-contract=off"], "lalign_units.hip": ["-ffp-contract=off"]}


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force=False, verbose=True):
    objdir = os.path.join(HERE, "..", "build")
    os.makedirs(objdir, exist_ok=True)
    headers = [os.path.abspath(__file__), os.path.join(CSRC, "common.h"), os.path.join(CSRC, "rowcfg.h"), os.path.join(CSRC, "coop.h"), os.path.join(CSRC, "recurrent.h"), os.path.join(CSRC, "ldsdma.h"), os.path.join(CSRC, "text_digits.h"), os.path.join(CSRC, "ctc_lattice.h"), os.path.join(CSRC, "moment_tiles.h"), os.path.join(CSRC, "dist_tile.h"), os.path.join(CSRC, "dtw_strip.h"), os.path.join(CSRC, "dtw_units_walk.h"), os.path.join(CSRC, "abx_rule.h"), os.path.join(CSRC, "sdtw_rule.h"), os.path.join(CSRC, "lalign_rule.h"), os.path.join(HERE, "..", "include", "cpc2_hip.h")]
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    if not force and _newer(LIB, srcs + headers):
        return LIB

    def compile_one(src):
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        if not force and _newer(obj, [src] + headers):
            return obj
        cmd = [HIPCC] + FLAGS + (DEVICE_FLAGS if src.endswith(".hip") else []) + FILE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        noise = [ln for ln in res.stdout.splitlines() if ln.strip() and "is not a recognized feature for this target" not in ln]
        if noise:
            print("\n".join(noise), flush=True)
        if res.returncode != 0:
            raise subprocess.CalledProcessError(res.returncode, cmd)
        return obj

    with ThreadPoolExecutor(max_workers=4) as pool:
        objs = list(pool.map(compile_one, srcs))
    cmd = [HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
