"""Diagnostic build of the HIP library: the same sources with -DSVLM_TUNING, i.e. WITH the environment-driven tuning switches
(SVLM_GEMM_BM, SVLM_PREFILL_SPLITS, SVLM_DA_DIAG, ...), the timing-only DIAG kernels and svlm_diag_last_gemm_plan, none of which the
product library contains.  __graft_entry__.build() builds the default one too (the GEMM path tests drive it); this tool is for
variants: SVLM_DIAG_DEFS adds -D flags (e.g. -DGEMM_DIAG=2) and then needs SVLM_DIAG_NAME, the variant library's own name.
    python tools/build_diag_lib.py        ->  streaming-vlm_amd/build/libsvlm_hip_diag.so
    SVLM_LIB_PATH=streaming-vlm_amd/build/libsvlm_hip_diag.so python tools/gemm_sweep.py ...
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import __graft_entry__ as g  # noqa: E402

print(g.build_diag(force="--force" in sys.argv, defs=os.environ.get("SVLM_DIAG_DEFS", "").split(),
                   name=os.environ.get("SVLM_DIAG_NAME", "libsvlm_hip_diag.so")))
