"""Build the NornicDB-AMD native kernel extension in-tree.

Usage:  python setup.py build_ext --inplace

Targets MI355X (gfx950) only. Cross-compiles fine on a GPU-less box.
"""
import os
import glob

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from setuptools import setup
from torch.utils.cpp_extension import BuildExtension, CUDAExtension

ROOT = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "nornicdb_amd", "csrc")

sources = sorted(
    s
    for s in glob.glob(os.path.join(CSRC, "*.cpp")) + glob.glob(os.path.join(CSRC, "*.hip"))
    # torch's hipify step writes generated copies named *_hip.hip; skip them.
    if not s.endswith("_hip.hip")
)

setup(
    name="nornicdb_amd",
    version="0.1.0",
    packages=["nornicdb_amd"],
    ext_modules=[
        CUDAExtension(
            name="nornicdb_amd._C",
            sources=sources,
            extra_compile_args={
                "cxx": ["-O3", "-std=c++17"],
                # kNN tile knobs of knn_mfma.hip: NORNICDB_KNN_RG is the
                # number of 4-wave row groups per workgroup (1 or 2, default
                # 2: one 8-wave workgroup per CU); NORNICDB_KNN_BM the rows
                # of one row group (experiment knob; default 160). A panel
                # is KNN_RG * KNN_BM rows. NORNICDB_KNN_STAGGER (0 or 1, with
                # KNN_RG = 2 only) runs row group 1 half a stage behind row
                # group 0.
                "nvcc": ["-O3", "-std=c++17"] + [
                    "-D" + macro + "=" + os.environ["NORNICDB_" + macro]
                    for macro in ("KNN_BM", "KNN_RG", "KNN_STAGGER")
                    if os.environ.get("NORNICDB_" + macro)],
            },
        )
    ],
    cmdclass={"build_ext": BuildExtension.with_options(use_ninja=True)},
)
