"""Builds the in-tree HIP extension ``libpwn_hip.so`` for gfx950 (hipcc cross-compiles without a GPU)."""
from __future__ import annotations

import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = [os.path.join(_HERE, "csrc", f) for f in ("pwn_hip_capi.hip", "pwn_buffers.h", "pwn_kernels.h", "pwn_math.h", "pwn_scene_kernels.h", "pwn_scene_capi.h", "pwn_stats.h", "pwn_consensus.h", "pwn_track.h", "pwn_track_capi.h")]
HEADER = os.path.join(os.path.dirname(_HERE), "include", "pwn_hip.h")
TEST_HEADER = os.path.join(os.path.dirname(_HERE), "include", "pwn_hip_testing.h")
OUT = os.path.join(_HERE, "libpwn_hip.so")
# -ffp-contract=off: the kernels reproduce the CPU path's evaluation order; a fused multiply-add would change bits.
# -fno-slp-vectorize: the SLP vectoriser pairs scalar fp32 ops into v_pk_*_f32 and pays for it in v_mov shuffles and registers
#   (k_corr_linearize 124 -> 98 VGPRs without it; same bits, +3 % whole-step throughput measured on MI355X).
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-fPIC", "-shared", "-pthread", "-Wall",
         "-Wno-unused-function"]


def build(force: bool = False, verbose: bool = False) -> str:
    deps = SOURCES + [HEADER, TEST_HEADER, __file__]
    stale = (not os.path.exists(OUT)) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps)
    if force or stale:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc] + FLAGS + ["-o", OUT, SOURCES[0]]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return OUT


def build_tools(force: bool = False) -> str:
    """The C++ harness over the host mirror (tools/pwn_hip_simple_aligner.cpp); plain g++, links libpwn_hip.so."""
    root = os.path.dirname(_HERE)
    src = os.path.join(root, "tools", "pwn_hip_simple_aligner.cpp")
    out = os.path.join(root, "tools", "pwn_hip_simple_aligner")
    deps = [src, os.path.join(_HERE, "host", "pwn_hip.hpp"), HEADER, OUT]
    if force or (not os.path.exists(out)) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src, "-o", out, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # the mapping loop of pwn_aligner.cpp (Cloud::add + Merger::merge + Cloud::save) over the same mirror
    src2 = os.path.join(root, "tools", "pwn_hip_scene_aligner.cpp")
    out2 = os.path.join(root, "tools", "pwn_hip_scene_aligner")
    deps2 = [src2] + deps[1:]
    if force or (not os.path.exists(out2)) or any(os.path.getmtime(d) > os.path.getmtime(out2) for d in deps2):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src2, "-o", out2, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # the tracker + closer flow (PwnTracker::processFrame, CloudCache, batched matchClouds, statistics, priors) over the same mirror
    src3 = os.path.join(root, "tools", "pwn_hip_tracker_app.cpp")
    out3 = os.path.join(root, "tools", "pwn_hip_tracker_app")
    deps3 = [src3] + deps[1:]
    if force or (not os.path.exists(out3)) or any(os.path.getmtime(d) > os.path.getmtime(out3) for d in deps3):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src3, "-o", out3, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # bench.py's workload driven from C++ (device and page-locked memory through the C-ABI: no HIP headers, no HIP runtime on the link line)
    src4 = os.path.join(root, "tools", "pwn_hip_bench.cpp")
    out4 = os.path.join(root, "tools", "pwn_hip_bench")
    deps4 = [src4] + deps[1:]
    if force or (not os.path.exists(out4)) or any(os.path.getmtime(d) > os.path.getmtime(out4) for d in deps4):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src4, "-o", out4, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # PwnMatcherBase::makeCloudBatch against makeCloud per frame, every downloaded array compared (exit status 0 = no difference)
    src6 = os.path.join(root, "tools", "pwn_hip_scaled_batch_check.cpp")
    out6 = os.path.join(root, "tools", "pwn_hip_scaled_batch_check")
    deps6 = [src6] + deps[1:]
    if force or (not os.path.exists(out6)) or any(os.path.getmtime(d) > os.path.getmtime(out6) for d in deps6):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src6, "-o", out6, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # PwnCloserWithMerger::processPartition of the C++ mirror against the relations the Python mirror wrote to a file (exit status 0 = no difference)
    src7 = os.path.join(root, "tools", "pwn_hip_merged_closure_check.cpp")
    out7 = os.path.join(root, "tools", "pwn_hip_merged_closure_check")
    deps7 = [src7] + deps[1:]
    if force or (not os.path.exists(out7)) or any(os.path.getmtime(d) > os.path.getmtime(out7) for d in deps7):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src7, "-o", out7, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # PwnMerger::mergeNodeList of the C++ mirror against the fused cloud the Python mirror wrote to a file (exit status 0 = equal byte for byte)
    src8 = os.path.join(root, "tools", "pwn_hip_merge_clouds_check.cpp")
    out8 = os.path.join(root, "tools", "pwn_hip_merge_clouds_check")
    deps8 = [src8] + deps[1:]
    if force or (not os.path.exists(out8)) or any(os.path.getmtime(d) > os.path.getmtime(out8) for d in deps8):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src8, "-o", out8, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # ManifoldVoronoiExtractor::process of the C++ mirror against the images the Python mirror wrote to a file (exit status 0 = equal byte for byte)
    src9 = os.path.join(root, "tools", "pwn_hip_manifold_check.cpp")
    out9 = os.path.join(root, "tools", "pwn_hip_manifold_check")
    deps9 = [src9] + deps[1:]
    if force or (not os.path.exists(out9)) or any(os.path.getmtime(d) > os.path.getmtime(out9) for d in deps9):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src9, "-o", out9, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # CloudCache(sceneReady) -> PwnMerger::mergeNodeList of the C++ mirror against the Python mirror's fused cloud, Stats and Gaussians included
    src10 = os.path.join(root, "tools", "pwn_hip_scene_ready_check.cpp")
    out10 = os.path.join(root, "tools", "pwn_hip_scene_ready_check")
    deps10 = [src10] + deps[1:]
    if force or (not os.path.exists(out10)) or any(os.path.getmtime(d) > os.path.getmtime(out10) for d in deps10):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src10, "-o", out10, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # "stop when converged" through the C++ mirror against the results and step traces the Python mirror wrote to a file (exit status 0 = equal bit for bit)
    src11 = os.path.join(root, "tools", "pwn_hip_early_stop_check.cpp")
    out11 = os.path.join(root, "tools", "pwn_hip_early_stop_check")
    deps11 = [src11] + deps[1:]
    if force or (not os.path.exists(out11)) or any(os.path.getmtime(d) > os.path.getmtime(out11) for d in deps11):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src11, "-o", out11, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # the closure records (Aligner::omega() computed on the device) through the C++ mirror against the bytes the Python mirror wrote to a file (exit status 0 = equal)
    src12 = os.path.join(root, "tools", "pwn_hip_closure_records_check.cpp")
    out12 = os.path.join(root, "tools", "pwn_hip_closure_records_check")
    deps12 = [src12] + deps[1:]
    if force or (not os.path.exists(out12)) or any(os.path.getmtime(d) > os.path.getmtime(out12) for d in deps12):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src12, "-o", out12, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # batch alignment with SE(3) priors through the C++ mirror against the records the Python mirror wrote to a file (exit status 0 = equal byte for byte)
    src13 = os.path.join(root, "tools", "pwn_hip_batch_priors_check.cpp")
    out13 = os.path.join(root, "tools", "pwn_hip_batch_priors_check")
    deps13 = [src13] + deps[1:]
    if force or (not os.path.exists(out13)) or any(os.path.getmtime(d) > os.path.getmtime(out13) for d in deps13):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src13, "-o", out13, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # SceneAligner (pwn_hip_scene_step per frame) through the C++ mirror against what the Python mirror wrote to a file (exit status 0 = equal byte for byte)
    src14 = os.path.join(root, "tools", "pwn_hip_scene_step_check.cpp")
    out14 = os.path.join(root, "tools", "pwn_hip_scene_step_check")
    deps14 = [src14] + deps[1:]
    if force or (not os.path.exists(out14)) or any(os.path.getmtime(d) > os.path.getmtime(out14) for d in deps14):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src14, "-o", out14, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # MapCloser::validatePartitions of the C++ mirror against the decisions and counters the Python mirror wrote to a file (exit status 0 = no difference)
    src15 = os.path.join(root, "tools", "pwn_hip_consensus_check.cpp")
    out15 = os.path.join(root, "tools", "pwn_hip_consensus_check")
    deps15 = [src15] + deps[1:]
    if force or (not os.path.exists(out15)) or any(os.path.getmtime(d) > os.path.getmtime(out15) for d in deps15):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src15, "-o", out15, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # PwnTrackerBatch::processFrames of the C++ mirror against the result records, states and key clouds the Python mirror wrote to a file (exit status 0 = equal bit for bit)
    src16 = os.path.join(root, "tools", "pwn_hip_track_streams_check.cpp")
    out16 = os.path.join(root, "tools", "pwn_hip_track_streams_check")
    deps16 = [src16] + deps[1:]
    if force or (not os.path.exists(out16)) or any(os.path.getmtime(d) > os.path.getmtime(out16) for d in deps16):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", root, src16, "-o", out16, "-L", _HERE, "-lpwn_hip",
                               "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd"])
    # PwnCloser::processPartition over the GPUs of a node in native code: the mirror + RCCL (broadcast of the flat `current` cloud, all-gather of the
    # match records); the program's own streams and events come from the HIP runtime
    src5 = os.path.join(root, "tools", "pwn_hip_partition_app.cpp")
    out5 = os.path.join(root, "tools", "pwn_hip_partition_app")
    deps5 = [src5] + deps[1:]
    if os.path.exists("/opt/rocm/include/rccl/rccl.h") and (force or (not os.path.exists(out5)) or any(os.path.getmtime(d) > os.path.getmtime(out5) for d in deps5)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", root, "-I", "/opt/rocm/include", src5, "-o", out5, "-L", _HERE, "-lpwn_hip",
                               "-L", "/opt/rocm/lib", "-lrccl", "-lamdhip64", "-Wl,-rpath,$ORIGIN/../g2o_frontend_amd", "-Wl,-rpath,/opt/rocm/lib"])
    return out


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_tools(force="--force" in sys.argv))
