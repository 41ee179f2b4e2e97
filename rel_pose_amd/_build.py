"""Build librelpose_hip.so, librelpose_readout.so, librelpose_eightpoint.so, librelpose_refine.so, librelpose_consensus.so, librelpose_submatch.so, librelpose_fivepoint.so, librelpose_homography.so, librelpose_triangulate.so, librelpose_conv5x5.so, librelpose_guided.so, librelpose_rotation.so, librelpose_select.so, librelpose_covariance.so and librelpose_resection.so (gfx950) in-tree with hipcc.  No CPU fallback exists: if the build or
the load fails, every op in rel_pose_amd raises."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librelpose_hip.so")
SOURCES = ["gemm.hip", "gemm_dma.hip", "rowwise.hip", "attention.hip", "attention_bf16.hip", "dw192_bf16.hip", "dw192_f32.hip", "dw192_split3.hip", "dx_lnbwd_bf16.hip", "emm.hip", "emm_bf16.hip", "batchnorm.hip", "se3loss.hip", "geom.hip", "augment.hip", "mlp_fused.hip", "linear_rows.hip", "conv_stem.hip", "conv_stem_bf16.hip", "conv_stem_wgrad_bf16.hip", "conv_stem_wgrad_f32.hip", "conv3x3_bf16.hip", "conv3x3_wgrad_bf16.hip", "conv3x3_wgrad_f32.hip", "conv3x3_f32.hip", "conv3x3_c128_f32.hip"]
# the readout library (include/relpose_readout.h): its own sources, outside csrc/ -- the hot path's source set stays what it was
READOUT_CSRC = os.path.join(HERE, "csrc_readout")
READOUT_LIB = os.path.join(HERE, "librelpose_readout.so")
READOUT_SOURCES = ["emm_readout.hip"]
# the eight-point library (include/relpose_eightpoint.h): the same pattern, a third library with sources of its own
EIGHTPOINT_CSRC = os.path.join(HERE, "csrc_eightpoint")
EIGHTPOINT_LIB = os.path.join(HERE, "librelpose_eightpoint.so")
EIGHTPOINT_SOURCES = ["eight_point.hip"]
# the refinement library (include/relpose_refine.h): a fourth library, the same pattern again
REFINE_CSRC = os.path.join(HERE, "csrc_refine")
REFINE_LIB = os.path.join(HERE, "librelpose_refine.so")
REFINE_SOURCES = ["refine_pose.hip"]
# the consensus library (include/relpose_consensus.h): a fifth library, the same pattern once more
CONSENSUS_CSRC = os.path.join(HERE, "csrc_consensus")
CONSENSUS_LIB = os.path.join(HERE, "librelpose_consensus.so")
CONSENSUS_SOURCES = ["consensus.hip"]
# the sub-token localisation library (include/relpose_submatch.h): a sixth library, the same pattern
SUBMATCH_CSRC = os.path.join(HERE, "csrc_submatch")
SUBMATCH_LIB = os.path.join(HERE, "librelpose_submatch.so")
SUBMATCH_SOURCES = ["submatch.hip"]
# the five-point consensus library (include/relpose_fivepoint.h): a seventh library, the same pattern
FIVEPOINT_CSRC = os.path.join(HERE, "csrc_fivepoint")
FIVEPOINT_LIB = os.path.join(HERE, "librelpose_fivepoint.so")
FIVEPOINT_SOURCES = ["five_point.hip"]
# the homography library (include/relpose_homography.h): an eighth library, the same pattern
HOMOGRAPHY_CSRC = os.path.join(HERE, "csrc_homography")
HOMOGRAPHY_LIB = os.path.join(HERE, "librelpose_homography.so")
HOMOGRAPHY_SOURCES = ["homography.hip"]
# the triangulation library (include/relpose_triangulate.h): a ninth library, the same pattern
TRIANGULATE_CSRC = os.path.join(HERE, "csrc_triangulate")
TRIANGULATE_LIB = os.path.join(HERE, "librelpose_triangulate.so")
TRIANGULATE_SOURCES = ["triangulate.hip"]
# the 5x5 input-gradient library (include/relpose_conv5x5.h): a tenth library, the same pattern; the one kernel of the hot path that
# lives outside csrc/ (the main library's surface stays what it was)
CONV5X5_CSRC = os.path.join(HERE, "csrc_conv5x5")
CONV5X5_LIB = os.path.join(HERE, "librelpose_conv5x5.so")
CONV5X5_SOURCES = ["conv5x5_dgrad_f32.hip"]
# the guided-matching library (include/relpose_guided.h): an eleventh library, the same pattern
GUIDED_CSRC = os.path.join(HERE, "csrc_guided")
GUIDED_LIB = os.path.join(HERE, "librelpose_guided.so")
GUIDED_SOURCES = ["emm_guided.hip"]
# the pure-rotation library (include/relpose_rotation.h): a twelfth library, the same pattern
ROTATION_CSRC = os.path.join(HERE, "csrc_rotation")
ROTATION_LIB = os.path.join(HERE, "librelpose_rotation.so")
ROTATION_SOURCES = ["rotation.hip"]
# the model-selection library (include/relpose_select.h): a thirteenth library, the same pattern
SELECT_CSRC = os.path.join(HERE, "csrc_select")
SELECT_LIB = os.path.join(HERE, "librelpose_select.so")
SELECT_SOURCES = ["select.hip"]
# the pose-covariance library (include/relpose_covariance.h): a fourteenth library, the same pattern; its 5 x 5 algebra is a header of its own
COVARIANCE_CSRC = os.path.join(HERE, "csrc_covariance")
COVARIANCE_LIB = os.path.join(HERE, "librelpose_covariance.so")
COVARIANCE_SOURCES = ["covariance.hip"]
# the resection library (include/relpose_resection.h): a fifteenth library, the same pattern
RESECTION_CSRC = os.path.join(HERE, "csrc_resection")
RESECTION_LIB = os.path.join(HERE, "librelpose_resection.so")
RESECTION_SOURCES = ["resection.hip"]
ARCH = "gfx950"


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return "hipcc"


def _stale(lib, csrc, sources, headers):
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    return any(os.path.getmtime(d) > t for d in [os.path.join(csrc, s) for s in sources] + headers)


def needs_build():
    return _stale(LIB, CSRC, SOURCES, _headers())


def readout_needs_build():
    return _stale(READOUT_LIB, READOUT_CSRC, READOUT_SOURCES, _readout_headers())


def eightpoint_needs_build():
    return _stale(EIGHTPOINT_LIB, EIGHTPOINT_CSRC, EIGHTPOINT_SOURCES, _eightpoint_headers())


def refine_needs_build():
    return _stale(REFINE_LIB, REFINE_CSRC, REFINE_SOURCES, _refine_headers())


def consensus_needs_build():
    return _stale(CONSENSUS_LIB, CONSENSUS_CSRC, CONSENSUS_SOURCES, _consensus_headers())


def submatch_needs_build():
    return _stale(SUBMATCH_LIB, SUBMATCH_CSRC, SUBMATCH_SOURCES, _submatch_headers())


def fivepoint_needs_build():
    return _stale(FIVEPOINT_LIB, FIVEPOINT_CSRC, FIVEPOINT_SOURCES, _fivepoint_headers())


def homography_needs_build():
    return _stale(HOMOGRAPHY_LIB, HOMOGRAPHY_CSRC, HOMOGRAPHY_SOURCES, _homography_headers())


def triangulate_needs_build():
    return _stale(TRIANGULATE_LIB, TRIANGULATE_CSRC, TRIANGULATE_SOURCES, _triangulate_headers())


def conv5x5_needs_build():
    return _stale(CONV5X5_LIB, CONV5X5_CSRC, CONV5X5_SOURCES, _conv5x5_headers())


def guided_needs_build():
    return _stale(GUIDED_LIB, GUIDED_CSRC, GUIDED_SOURCES, _guided_headers())


def rotation_needs_build():
    return _stale(ROTATION_LIB, ROTATION_CSRC, ROTATION_SOURCES, _rotation_headers())


def select_needs_build():
    return _stale(SELECT_LIB, SELECT_CSRC, SELECT_SOURCES, _select_headers())


def covariance_needs_build():
    return _stale(COVARIANCE_LIB, COVARIANCE_CSRC, COVARIANCE_SOURCES, _covariance_headers())


def resection_needs_build():
    return _stale(RESECTION_LIB, RESECTION_CSRC, RESECTION_SOURCES, _resection_headers())


def build(force=False, verbose=True):
    """Compile under an exclusive file lock (eight ranks of a first `torchrun` would otherwise write the same .o / .so at
    once) and move the finished library into place atomically, so a concurrent loader never maps a half-written file.
    All fifteen libraries are built under the one lock, each only if it is stale (force: all, every translation unit)."""
    import fcntl
    with open(os.path.join(HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if force or needs_build():               # (not stale any more: another rank built it while this one waited)
                _build_locked(verbose, force, LIB, CSRC, SOURCES, _headers())
            if force or readout_needs_build():
                _build_locked(verbose, force, READOUT_LIB, READOUT_CSRC, READOUT_SOURCES, _readout_headers())
            if force or eightpoint_needs_build():
                _build_locked(verbose, force, EIGHTPOINT_LIB, EIGHTPOINT_CSRC, EIGHTPOINT_SOURCES, _eightpoint_headers())
            if force or refine_needs_build():
                _build_locked(verbose, force, REFINE_LIB, REFINE_CSRC, REFINE_SOURCES, _refine_headers())
            if force or consensus_needs_build():
                _build_locked(verbose, force, CONSENSUS_LIB, CONSENSUS_CSRC, CONSENSUS_SOURCES, _consensus_headers())
            if force or submatch_needs_build():
                _build_locked(verbose, force, SUBMATCH_LIB, SUBMATCH_CSRC, SUBMATCH_SOURCES, _submatch_headers())
            if force or fivepoint_needs_build():
                _build_locked(verbose, force, FIVEPOINT_LIB, FIVEPOINT_CSRC, FIVEPOINT_SOURCES, _fivepoint_headers())
            if force or homography_needs_build():
                _build_locked(verbose, force, HOMOGRAPHY_LIB, HOMOGRAPHY_CSRC, HOMOGRAPHY_SOURCES, _homography_headers())
            if force or triangulate_needs_build():
                _build_locked(verbose, force, TRIANGULATE_LIB, TRIANGULATE_CSRC, TRIANGULATE_SOURCES, _triangulate_headers())
            if force or conv5x5_needs_build():
                _build_locked(verbose, force, CONV5X5_LIB, CONV5X5_CSRC, CONV5X5_SOURCES, _conv5x5_headers())
            if force or guided_needs_build():
                _build_locked(verbose, force, GUIDED_LIB, GUIDED_CSRC, GUIDED_SOURCES, _guided_headers())
            if force or rotation_needs_build():
                _build_locked(verbose, force, ROTATION_LIB, ROTATION_CSRC, ROTATION_SOURCES, _rotation_headers())
            if force or select_needs_build():
                _build_locked(verbose, force, SELECT_LIB, SELECT_CSRC, SELECT_SOURCES, _select_headers())
            if force or covariance_needs_build():
                _build_locked(verbose, force, COVARIANCE_LIB, COVARIANCE_CSRC, COVARIANCE_SOURCES, _covariance_headers())
            if force or resection_needs_build():
                _build_locked(verbose, force, RESECTION_LIB, RESECTION_CSRC, RESECTION_SOURCES, _resection_headers())
            return LIB
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _headers():
    return [os.path.join(CSRC, h) for h in sorted(os.listdir(CSRC)) if h.endswith(".h")] + \
           [os.path.join(os.path.dirname(HERE), "include", "relpose_hip.h")]


def _readout_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_readout.h")]


def _eightpoint_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_eightpoint.h")]


def _refine_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_refine.h")]


def _consensus_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_consensus.h")]


def _submatch_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_submatch.h")]


def _fivepoint_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_fivepoint.h")]


def _homography_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_homography.h")]


def _triangulate_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_triangulate.h")]


def _conv5x5_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_conv5x5.h")]


def _guided_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_guided.h")]


def _rotation_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_rotation.h")]


def _select_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_select.h")]


def _covariance_headers():
    return _headers() + [os.path.join(COVARIANCE_CSRC, "sym5.h"), os.path.join(os.path.dirname(HERE), "include", "relpose_covariance.h")]


def _resection_headers():
    return _headers() + [os.path.join(os.path.dirname(HERE), "include", "relpose_resection.h")]


def _build_locked(verbose, force, lib, csrc, sources, headers):
    """force: every translation unit is recompiled; otherwise only objects older than their source or any header."""
    cc = _hipcc()
    objs = []
    procs = []
    hdr_t = max(os.path.getmtime(h) for h in headers)
    for s in sources:
        o = os.path.join(csrc, s.replace(".hip", ".o"))
        objs.append(o)
        if not force and os.path.exists(o) and os.path.getmtime(o) > max(hdr_t, os.path.getmtime(os.path.join(csrc, s))):
            continue
        cmd = [cc, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-c", os.path.join(csrc, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError("hipcc failed on " + s)
    tmp = lib + ".tmp.%d" % os.getpid()
    cmd = [cc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, lib)
    return lib


if __name__ == "__main__":
    build(force="--force" in sys.argv)
