"""Build the bloombee_amd gfx950 HIP extension in-tree.

Invokes hipcc directly (native HIP source — no hipify pass, no CUDA
compatibility layer). The built .so lands at bloombee_amd/ops/_hip_ops.so so
it travels with the repo snapshot to the GPU box (gpurun ships in-tree .so
files; a JIT cache under ~/.cache would not).

Usage:
    python setup.py build_ext --inplace     # or: python setup.py hip
"""
import os
import subprocess
import sys
import sysconfig
from pathlib import Path

ROOT = Path(__file__).resolve().parent
HIP_DIR = ROOT / "bloombee_amd" / "ops" / "hip"
OUT_SO = ROOT / "bloombee_amd" / "ops" / "_hip_ops.so"
W8_SO = ROOT / "bloombee_amd" / "ops" / "_hip_w8.so"
RING_SO = ROOT / "bloombee_amd" / "ops" / "_hip_ring.so"
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def torch_paths():
    import torch

    tdir = Path(torch.__file__).parent
    return tdir / "include", tdir / "lib"


def _torch_ext_flags(name: str) -> list:
    tinc, _ = torch_paths()
    return [
        "-I", str(tinc),
        "-I", str(tinc / "torch" / "csrc" / "api" / "include"),
        "-I", "/opt/rocm/include",
        "-I", sysconfig.get_paths()["include"],
        "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", "-DHIPBLAS_V2",
        "-DCUDA_HAS_FP16=1", "-D__HIP_NO_HALF_OPERATORS__=1",
        "-D__HIP_NO_HALF_CONVERSIONS__=1", "-DHIP_ENABLE_WARP_SYNC_BUILTINS=1",
        "-DTORCH_API_INCLUDE_EXTENSION_H", f"-DTORCH_EXTENSION_NAME={name}",
    ]


def _link(objs, out: Path) -> list:
    _, tlib = torch_paths()
    return [
        "g++", "-shared", *map(str, objs),
        "-L", str(tlib), "-L", "/opt/rocm/lib",
        "-lc10", "-ltorch", "-ltorch_cpu", "-ltorch_python",
        "-lamdhip64", "-lc10_hip", "-ltorch_hip", "-lz",
        "-o", str(out),
    ]


def _run(cmds, verbose: bool) -> None:
    for cmd in cmds:
        if verbose:
            print("+", " ".join(cmd), file=sys.stderr)
        subprocess.run(cmd, check=True)


def build_w8(verbose: bool = True) -> Path:
    """_hip_w8.so: the fp8 (e4m3) weight tier, bindings (w8_ext.hip) and
    kernels (gemm_w8.hip, gemm_w8_tiled.hip) in one translation unit, built without packed-fp32
    instructions."""
    obj = HIP_DIR / "w8_ext.o"
    compile_cmd = [
        "/opt/rocm/bin/hipcc", f"--offload-arch={ARCH}",
        "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
        "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
        *_torch_ext_flags("_hip_w8"),
        "-c", str(HIP_DIR / "w8_ext.hip"), "-o", str(obj),
    ]
    _run((compile_cmd, _link([obj], W8_SO)), verbose)
    obj.unlink(missing_ok=True)
    return W8_SO


def build_ring(verbose: bool = True) -> Path:
    """_hip_ring.so: the ring-attention fold, bindings (ring_ext.hip) and
    kernel (attn_ring.hip) in one translation unit."""
    obj = HIP_DIR / "ring_ext.o"
    compile_cmd = [
        "/opt/rocm/bin/hipcc", f"--offload-arch={ARCH}",
        "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
        *_torch_ext_flags("_hip_ring"),
        "-c", str(HIP_DIR / "ring_ext.hip"), "-o", str(obj),
    ]
    _run((compile_cmd, _link([obj], RING_SO)), verbose)
    obj.unlink(missing_ok=True)
    return RING_SO


def build(verbose: bool = True) -> Path:
    src = HIP_DIR / "ext.hip"
    obj = HIP_DIR / "ext.o"
    # the fp8 KV kernels are a translation unit of their own (raw-pointer
    # launchers, no torch headers), built without packed-fp32 instructions
    kv8_src = HIP_DIR / "kv_fp8.hip"
    kv8_obj = HIP_DIR / "kv_fp8.o"
    hipcc = [
        "/opt/rocm/bin/hipcc",
        f"--offload-arch={ARCH}",
        "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc",
    ]
    kv8_cmd = hipcc + [
        "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
        "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__=1",
        "-c", str(kv8_src), "-o", str(kv8_obj),
    ]
    compile_cmd = hipcc + _torch_ext_flags("_hip_ops") + [
        "-c", str(src), "-o", str(obj),
    ]
    _run((compile_cmd, kv8_cmd, _link([obj, kv8_obj], OUT_SO)), verbose)
    obj.unlink(missing_ok=True)
    kv8_obj.unlink(missing_ok=True)
    build_w8(verbose)
    build_ring(verbose)
    return OUT_SO


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("hip", "build_ext"):
        build()
    else:
        print(__doc__)
