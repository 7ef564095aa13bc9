"""Builds the HIP libraries in-tree for gfx950 (hipcc cross-compiles without a GPU).

    python -m spadot_amd.csrc.build [--force]

One shared object per .hip translation unit, written next to its source so that it travels
with the repository snapshot to the GPU box.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ARCH = "gfx950"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# shared object -> translation units
TARGETS = {
    "libspadot_ot.so": ["ot_sinkhorn.hip", "ot_cost.hip", "ot_small.hip"],
    "libspadot_model.so": ["model_kernels.hip", "gat_mfma.hip", "gemm_bf16.hip", "gemm_wgrad_bf16.hip", "mlp_chain.hip", "gat_tail.hip", "enc_fused.hip", "recon_fb.hip", "preprocess.hip", "sctransform.hip", "markers.hip", "silhouette.hip", "trends.hip", "gmm.hip", "nhood.hip", "cooccur.hip", "autocorr.hip", "ligrec.hip", "localmoran.hip", "crossmoran.hip", "ripley.hip", "correlogram.hip", "embed.hip", "sepal.hip", "territories.hip", "hops.hip"],
}

# per-source extra flags.  ot_sinkhorn: the fused pass keeps its whole register budget (256 VGPRs) for the row band;
# machine LICM hoists the 64-bit polynomial constants of the inlined log/exp out of the sweep loop into VGPR pairs
# and then SPILLS them (scratch reloads queue behind the prefetch in the vmcnt FIFO), so it is switched off there.
EXTRA = {"ot_sinkhorn.hip": ["-mllvm", "-disable-machine-licm"]}

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-Wno-unused-result", "-Wno-pass-failed"]


def _stale(src, out, extra_deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in [src, os.path.abspath(__file__)] + extra_deps if os.path.exists(d))


def build_all(force=False, verbose=True):
    inc = os.path.join(HERE, "..", "..", "include")
    headers = [os.path.join(inc, f) for f in os.listdir(inc)] if os.path.isdir(inc) else []
    headers += [os.path.join(HERE, f) for f in os.listdir(HERE) if f.endswith(".h")]       # csrc's own shared headers
    built, jobs, links = [], [], []
    defs = os.environ.get("SPADOT_BUILD_DEFS", "").split()      # e.g. "-DAGG_RING=4" (A/B builds on the GPU box)
    for out, srcs in TARGETS.items():
        o = os.path.join(HERE, out)
        paths = [os.path.join(HERE, s) for s in srcs]
        if force or any(_stale(s, o, headers) for s in paths):
            objs = []
            for s, name in zip(paths, srcs):          # one object per translation unit, then one link
                obj = s[:-4] + ".o"
                if force or _stale(s, obj, headers):
                    jobs.append([HIPCC] + [f for f in FLAGS if f != "-shared"] + EXTRA.get(name, []) + defs + ["-c", "-o", obj, s])
                objs.append(obj)
            links.append([HIPCC, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", o] + objs)
        built.append(o)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    if jobs:                                          # translation units are independent: compile them side by side
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=min(len(jobs), int(os.environ.get("SPADOT_BUILD_JOBS", "4")))) as ex:
            list(ex.map(run, jobs))
    for cmd in links:
        run(cmd)
    return built


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
