"""Builds cpupathtrace_amd/libpathtrace_hip.so (HIP kernels + C ABI) for gfx950, in-tree, with hipcc."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpathtrace_hip.so")
SOURCES = ["pt_api.cpp", "pt_meshes.cpp", "pt_pose.cpp", "pt_deform.cpp", "pt_morph.cpp", "pt_relight.cpp", "pt_motion.cpp", "pt_motion_shapes.cpp", "pt_query.cpp", "pt_gather.cpp", "pt_light_probes.cpp", "pt_radiance.cpp", "pt_light_passes.cpp", "pt_nearest.cpp", "pt_render.cpp", "pt_frames.cpp", "pt_frame_maps.cpp", "pt_checkpoint.cpp", "pt_checkpoint_format.cpp", "pt_image.cpp", "pt_bvh.cpp", "pt_build.hip", "pt_mesh.hip", "pt_mesh_batch.hip", "pt_deform.hip", "pt_relight.hip", "pt_post.hip", "pt_path.hip", "pt_walks.hip", "pt_nearest.hip", "pt_frame.hip", "pt_checkpoint.hip", "pt_denoise.hip"]
HEADERS = ["pt_host.h", "pt_sample_host.h", "pt_frames.h", "pt_checkpoint_format.h", "pt_checkpoint_kernels.h", "pt_checkpoint_launch.h", "pt_build.h", "pt_mesh.h", "pt_mesh_batch.h", "pt_mesh_batch_kernels.h", "pt_skin.h", "pt_deform_kernels.h", "pt_morph_skin.h", "pt_morph_rows.h", "pt_morph_kernels.h", "pt_relight_kernels.h", "pt_motion_shapes_kernels.h", "pt_query_kernels.h", "pt_sample_walk.h", "pt_gather_kernels.h", "pt_light_probe_kernels.h", "pt_radiance_kernels.h", "pt_light_pass_kernels.h", "pt_nearest_kernels.h", "pt_post.h", "pt_denoise.h", "pt_types.h", "pt_kernels.h", "pt_device.h", "pt_shading.h", "pt_trace.h", "pt_libm.h", "pt_bvh.h", "pt_noise.h", os.path.join("..", "..", "include", "pt_hip.h"),
           os.path.join("..", "..", "include", "pt_frame_noise.h"), os.path.join("..", "..", "include", "pt_frame_variance.h"), os.path.join("..", "..", "include", "pt_features.h"), os.path.join("..", "..", "include", "pt_checkpoint.h"),
           os.path.join("..", "..", "include", "pt_mesh.h"), os.path.join("..", "..", "include", "pt_pose.h"), os.path.join("..", "..", "include", "pt_deform.h"), os.path.join("..", "..", "include", "pt_morph.h"),os.path.join("..", "..", "include", "pt_motion.h"), os.path.join("..", "..", "include", "pt_motion_shapes.h"), os.path.join("..", "..", "include", "pt_query.h"), os.path.join("..", "..", "include", "pt_gather.h"), os.path.join("..", "..", "include", "pt_light_probes.h"), os.path.join("..", "..", "include", "pt_radiance.h"), os.path.join("..", "..", "include", "pt_light_passes.h"), os.path.join("..", "..", "include", "pt_nearest.h"),os.path.join("..", "..", "include", "pt_relight.h")]

# -ffp-contract=off + correctly rounded divide/sqrt: every fp32/fp64 operation is the IEEE operation the reference's
# x86-64 build performs (parity is bit-level); -O3 otherwise.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
         "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wall", "-Wno-unused-function", "-pthread"]


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def up_to_date():
    if not os.path.exists(LIB):
        return False
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force=False, verbose=False):
    """Compile the library unless it is up to date.  Safe when several processes (the ranks of a multi-GPU run) call it at once:
    one of them compiles, into a temporary file that is renamed into place, the others wait for the lock and find the result."""
    if not force and up_to_date():
        return LIB
    import fcntl
    with open(LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and up_to_date():
                return LIB
            tmp = "%s.%d.tmp" % (LIB, os.getpid())
            cmd = [hipcc()] + FLAGS + ["-x", "hip"] + [os.path.join(CSRC, f) for f in SOURCES] + ["-o", tmp]
            if verbose:
                print(" ".join(cmd))
            try:
                subprocess.run(cmd, check=True)
                os.replace(tmp, LIB)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
