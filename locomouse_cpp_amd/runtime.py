"""ctypes binding of liblocomouse_hip.so (the C-ABI in include/locomouse_hip.h).

This is how tests and bench.py drive the HIP path.  There is no CPU fallback:
if the shared library is missing or no HIP device is present, Context()
raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from .abi import (BB_FRAME_DTYPE, CALIB_RECORD_DTYPE, LM_ENC_GRAY8, LM_ENC_RGB24, LM_OK, lm_batch_result, lm_bb_result,
                  lm_calib_fit_result, lm_calib_opts, lm_calib_record, lm_enc_mark, lm_enc_overlay, lm_enc_result,
                  lm_enc_stats, lm_geometry, lm_jpeg_info, lm_jpeg_interval_stats, lm_jpeg_stats, lm_train_heldout,
                  lm_train_point, lm_train_problem, lm_train_stats, result_to_numpy)

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
LIB_PATH = os.path.join(PKG, "liblocomouse_hip.so")
CSRC = os.path.join(PKG, "csrc")

EXPORTED = (
    "lm_abi_version", "lm_last_error", "lm_ctx_create", "lm_ctx_destroy", "lm_get_geometry", "lm_ctx_stream",
    "lm_detect_batch", "lm_detect_batch_device", "lm_ctx_set_debug", "lm_debug_scores", "lm_debug_tail_mask",
    "lm_debug_kernel_times", "lm_debug_kernel_spans", "lm_synth_frames_device",
    "lm_bb_create", "lm_bb_destroy", "lm_bb_push", "lm_bb_push_device", "lm_bb_finish", "lm_bb_debug_binary",
    "lm_bb_stream", "lm_host_alloc", "lm_host_free",
    "lm_detect_submit", "lm_detect_submit_device", "lm_detect_collect", "lm_ctx_lanes", "lm_ctx_pending",
    "lm_debug_corr_work", "lm_debug_batch_slots", "lm_debug_dark_tile_width",
    "lm_debug_dark_tile_height", "lm_debug_tail_work", "lm_debug_tail_tiles", "lm_debug_point_work",
    "lm_debug_point_tiles", "lm_debug_screen_fallback", "lm_debug_narrow_work", "lm_debug_narrow_entries",
)

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-slp-vectorize",
               "-fvisibility=hidden", "-Wall", "-Wno-unused-function", "-Wno-unused-variable"]


HOST_DIR = os.path.join(PKG, "host")
HOST_LIB_PATH = os.path.join(PKG, "liblocomouse_host.so")
CLI_PATH = os.path.join(PKG, "bin", "LocoMouse")


# translation units of liblocomouse_hip.so
HIP_UNITS = ("lm_runtime.hip", "lm_corr.hip", "lm_bbox.hip", "lm_jpeg.hip", "lm_bkg.hip", "lm_jpeg_enc.hip",
             "lm_train.hip", "lm_calib.hip")

# include/locomouse_jpeg.h (device MJPEG decode), same library
JPEG_EXPORTED = ("lm_jpeg_create", "lm_jpeg_destroy", "lm_jpeg_decode_device", "lm_jpeg_probe", "lm_jpeg_stream",
                 "lm_jpeg_debug_stats", "lm_jpeg_device_alloc", "lm_jpeg_device_free", "lm_jpeg_upload",
                 "lm_jpeg_set_interval_path", "lm_jpeg_debug_interval_stats")

# include/locomouse_bkg.h (the background as a per-pixel temporal median), same library
BKG_EXPORTED = ("lm_bkg_create", "lm_bkg_destroy", "lm_bkg_push", "lm_bkg_push_device", "lm_bkg_finish",
                "lm_bkg_reset", "lm_bkg_samples", "lm_bkg_stream")
BKG_CLI_PATH = os.path.join(PKG, "bin", "LocoMouseBackground")

# include/locomouse_encode.h (device JPEG encode and the track overlay), same library
ENC_EXPORTED = ("lm_enc_slot_bytes", "lm_enc_slot_bytes_restart", "lm_enc_create", "lm_enc_create_restart", "lm_enc_destroy",
                "lm_enc_encode_device", "lm_enc_encode", "lm_enc_set_overlay", "lm_enc_render_encode_device", "lm_enc_render_encode", "lm_enc_render_device", "lm_enc_stream",
                "lm_enc_last_stats")

# include/locomouse_train.h (detector weights trained from labelled patches), same library
TRAIN_EXPORTED = ("lm_train_create", "lm_train_destroy", "lm_train_add_patches", "lm_train_gather",
                  "lm_train_gather_device", "lm_train_samples", "lm_train_reset", "lm_train_patches", "lm_train_solve",
                  "lm_train_margins", "lm_train_stream", "lm_train_set_groups", "lm_train_solve_many",
                  "lm_train_problem_block")
TRAIN_CLI_PATH = os.path.join(PKG, "bin", "LocoMouseTrain")
TRANSCODE_CLI_PATH = os.path.join(PKG, "bin", "LocoMouseTranscode")

# include/locomouse_calib.h (the two-view calibration map estimated from a marker video), same library
CALIB_EXPORTED = ("lm_calib_default_opts", "lm_calib_create", "lm_calib_destroy", "lm_calib_set_background", "lm_calib_push",
                  "lm_calib_push_device", "lm_calib_frames", "lm_calib_read", "lm_calib_reset", "lm_calib_stream",
                  "lm_calib_fit", "lm_calib_map")
CALIB_CLI_PATH = os.path.join(PKG, "bin", "LocoMouseCalibrate")

# include/locomouse_match.h (the bottom crop matched to a reference image's histogram), same library
MATCH_EXPORTED = ("lm_match_cdf", "lm_ctx_create_matched", "lm_debug_match_hist", "lm_debug_match_table",
                  "lm_debug_match_crop")


def _up_to_date(obj, cmd):
    """True when obj was built by the same command and is newer than every
    file its dependency list (hipcc -MMD) names."""
    try:
        with open(obj + ".cmd") as fh:
            if fh.read() != " ".join(cmd):
                return False
        with open(obj + ".d") as fh:
            deps = fh.read().replace("\\\n", " ").split(":", 1)[1].split()
        t = os.path.getmtime(obj)
        return all(os.path.getmtime(d) <= t for d in deps)
    except (OSError, IndexError):
        return False


def build(verbose=False, defines=(), out=None):
    """Compile liblocomouse_hip.so for gfx950 in-tree (hipcc cross-compiles
    without a GPU), then the host C++ LocoMouse mirror above it.  The
    translation units compile in parallel, then link into one library.
    `defines` / `out`: experiment builds (-D flags, another output path; the
    host mirror is then not rebuilt)."""
    objdir = os.path.join(ROOT, "build", "hip" if out is None else "hip_" + os.path.basename(out))
    os.makedirs(objdir, exist_ok=True)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *["-D" + d for d in defines]]
    flags = [f for f in HIPCC_FLAGS if f != "-shared"]
    procs, objs = [], []
    for u in HIP_UNITS:
        o = os.path.join(objdir, u.replace(".hip", ".o"))
        cmd = ["hipcc", *flags, *inc, "-c", "-MMD", "-MF", o + ".d", "-o", o, os.path.join(CSRC, u)]
        objs.append(o)
        if _up_to_date(o, cmd):
            continue
        if verbose:
            print(" ".join(cmd))
        procs.append((subprocess.Popen(cmd), cmd, o))
    for p, cmd, o in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
        with open(o + ".cmd", "w") as fh:
            fh.write(" ".join(cmd))
    target = out or LIB_PATH
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target, *objs]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    if out is None:
        build_host(verbose)
    return target


def build_host(verbose=False):
    """liblocomouse_host.so: the LocoMouse / Candidate / P22D / MyMat C++
    surface (locomouse_cpp_amd/host) linked against the C-ABI library."""
    srcs = [os.path.join(HOST_DIR, f)
            for f in ("LocoMouse.cpp", "Tracks.cpp", "match2nd.cpp", "FileStorage.cpp", "Media.cpp", "Jpeg.cpp", "Debug.cpp",
                      "Background.cpp", "JpegEncode.cpp", "Preview.cpp", "Inputs.cpp", "Train.cpp", "Calibration.cpp")]
    flags = ["g++", "-O3", "-std=c++17", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
             "-I" + HOST_DIR]
    cmd = [*flags, "-fPIC", "-shared", "-o", HOST_LIB_PATH, *srcs, "-L" + PKG, "-llocomouse_hip", "-lz",
           "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # the reference's command-line program (main.cpp), SURVEY.md §8(f) row 2
    os.makedirs(os.path.dirname(CLI_PATH), exist_ok=True)
    cmd = [*flags, "-o", CLI_PATH, os.path.join(HOST_DIR, "Cli.cpp"), "-L" + PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # LocoMouseBackground video.avi out.png [stride [permille]]: the background image the program above takes
    cmd = [*flags, "-o", BKG_CLI_PATH, os.path.join(HOST_DIR, "BackgroundCli.cpp"), "-L" + PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # LocoMouseTrain: detector weights (a model.yml) trained from labelled frames (host/Train.hpp)
    cmd = [*flags, "-o", TRAIN_CLI_PATH, os.path.join(HOST_DIR, "TrainCli.cpp"), "-L" + PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # LocoMouseTranscode: a video written again as grey MJPEG with restart markers (the device decoder's interval path)
    cmd = [*flags, "-o", TRANSCODE_CLI_PATH, os.path.join(HOST_DIR, "TranscodeCli.cpp"), "-L" + PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    # LocoMouseCalibrate: the calibration.yml estimated from a marker video (host/Calibration.hpp)
    cmd = [*flags, "-o", CALIB_CLI_PATH, os.path.join(HOST_DIR, "CalibrateCli.cpp"), "-L" + PKG, "-llocomouse_host",
           "-llocomouse_hip", "-Wl,-rpath,$ORIGIN/.."]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return HOST_LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        # torch ships its own libamdhip64.so.7 (same soname as /opt/rocm's):
        # load it first so this library and torch share one HIP runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run locomouse_cpp_amd.runtime.build() (no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        L.lm_abi_version.restype = C.c_int32
        L.lm_last_error.restype = C.c_char_p
        L.lm_ctx_create.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_ctx_destroy.argtypes = [C.c_void_p]
        L.lm_get_geometry.argtypes = [C.c_void_p, C.POINTER(lm_geometry)]
        L.lm_ctx_stream.argtypes = [C.c_void_p]
        L.lm_ctx_stream.restype = C.c_void_p
        for fn in (L.lm_detect_batch, L.lm_detect_batch_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                           C.POINTER(lm_batch_result)]
        for fn in (L.lm_detect_submit, L.lm_detect_submit_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.lm_detect_collect.argtypes = [C.c_void_p, C.POINTER(lm_batch_result)]
        for fn in (L.lm_ctx_lanes, L.lm_ctx_pending):
            fn.argtypes = [C.c_void_p]
            fn.restype = C.c_int32
        L.lm_ctx_set_debug.argtypes = [C.c_void_p, C.c_int32]
        L.lm_debug_scores.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.lm_debug_tail_mask.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.lm_debug_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.c_int32]
        L.lm_debug_kernel_times.restype = C.c_int32
        L.lm_debug_kernel_spans.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double), C.c_int32]
        L.lm_debug_kernel_spans.restype = C.c_int32
        L.lm_debug_corr_work.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.lm_debug_tail_work.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.lm_debug_tail_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.lm_debug_point_work.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.lm_debug_point_tiles.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.lm_debug_screen_fallback.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.lm_debug_narrow_work.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.lm_debug_narrow_entries.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                              C.POINTER(C.c_int32)]
        L.lm_debug_batch_slots.argtypes = [C.c_void_p]
        L.lm_debug_batch_slots.restype = C.c_int32
        L.lm_synth_frames_device.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                             C.c_int64]
        L.lm_bb_create.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_bb_destroy.argtypes = [C.c_void_p]
        for fn in (L.lm_bb_push, L.lm_bb_push_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.lm_bb_finish.argtypes = [C.c_void_p, C.POINTER(lm_bb_result)]
        L.lm_bb_debug_binary.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        L.lm_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
        L.lm_host_free.argtypes = [C.c_void_p]
        L.lm_bb_stream.argtypes = [C.c_void_p]
        L.lm_bb_stream.restype = C.c_void_p
        L.lm_jpeg_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_jpeg_destroy.argtypes = [C.c_void_p]
        L.lm_jpeg_decode_device.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int32,
                                            C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
        L.lm_jpeg_probe.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(lm_jpeg_info)]
        L.lm_jpeg_stream.argtypes = [C.c_void_p]
        L.lm_jpeg_stream.restype = C.c_void_p
        L.lm_jpeg_debug_stats.argtypes = [C.c_void_p, C.POINTER(lm_jpeg_stats)]
        L.lm_jpeg_set_interval_path.argtypes = [C.c_void_p, C.c_int32]
        L.lm_jpeg_debug_interval_stats.argtypes = [C.c_void_p, C.POINTER(lm_jpeg_interval_stats)]
        L.lm_bkg_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_bkg_destroy.argtypes = [C.c_void_p]
        for fn in (L.lm_bkg_push, L.lm_bkg_push_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.lm_bkg_finish.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.lm_bkg_reset.argtypes = [C.c_void_p]
        L.lm_bkg_samples.argtypes = [C.c_void_p]
        L.lm_bkg_samples.restype = C.c_int64
        L.lm_bkg_stream.argtypes = [C.c_void_p]
        L.lm_bkg_stream.restype = C.c_void_p
        L.lm_enc_slot_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        L.lm_enc_slot_bytes.restype = C.c_int64
        L.lm_enc_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_enc_slot_bytes_restart.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.lm_enc_slot_bytes_restart.restype = C.c_int64
        L.lm_enc_create_restart.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(C.c_void_p)]
        L.lm_enc_destroy.argtypes = [C.c_void_p]
        for fn in (L.lm_enc_encode_device, L.lm_enc_encode):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(lm_enc_result)]
        L.lm_enc_set_overlay.argtypes = [C.c_void_p, C.POINTER(lm_enc_overlay)]
        for fn in (L.lm_enc_render_encode_device, L.lm_enc_render_encode):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(lm_enc_result)]
        L.lm_enc_render_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.lm_enc_stream.argtypes = [C.c_void_p]
        L.lm_enc_stream.restype = C.c_void_p
        L.lm_enc_last_stats.argtypes = [C.c_void_p, C.POINTER(lm_enc_stats)]
        L.lm_train_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.lm_train_destroy.argtypes = [C.c_void_p]
        L.lm_train_add_patches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
        for fn in (L.lm_train_gather, L.lm_train_gather_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32]
        L.lm_train_samples.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.lm_train_reset.argtypes = [C.c_void_p]
        L.lm_train_patches.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.lm_train_solve.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_void_p,
                                     C.POINTER(C.c_double), C.POINTER(lm_train_stats)]
        L.lm_train_margins.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
        L.lm_train_stream.argtypes = [C.c_void_p]
        L.lm_train_set_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.lm_train_solve_many.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.lm_train_problem_block.argtypes = [C.c_void_p]
        L.lm_train_problem_block.restype = C.c_int32
        L.lm_train_stream.restype = C.c_void_p
        L.lm_calib_default_opts.argtypes = [C.POINTER(lm_calib_opts)]
        L.lm_calib_default_opts.restype = None
        L.lm_calib_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(lm_calib_opts),
                                      C.POINTER(C.c_void_p)]
        L.lm_calib_destroy.argtypes = [C.c_void_p]
        L.lm_calib_set_background.argtypes = [C.c_void_p, C.c_void_p]
        for fn in (L.lm_calib_push, L.lm_calib_push_device):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
        L.lm_calib_frames.argtypes = [C.c_void_p]
        L.lm_calib_frames.restype = C.c_int64
        L.lm_calib_read.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
        L.lm_calib_reset.argtypes = [C.c_void_p]
        L.lm_calib_stream.argtypes = [C.c_void_p]
        L.lm_calib_stream.restype = C.c_void_p
        L.lm_calib_fit.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(lm_calib_opts),
                                   C.c_int32, C.c_double, C.POINTER(lm_calib_fit_result)]
        L.lm_calib_map.argtypes = [C.POINTER(lm_calib_fit_result), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
        L.lm_match_cdf.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p]
        L.lm_ctx_create_matched.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.POINTER(C.c_void_p)]
        L.lm_debug_match_hist.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.lm_debug_match_table.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.lm_debug_match_crop.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
        _lib = L
    return _lib


class LMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"lm status {code}: {msg}")
        self.code = code


def _check(rc):
    if rc != LM_OK:
        raise LMError(rc, lib().lm_last_error().decode())


def synth_frames_device(d_ptr, rows, cols, first, n, pitch, device=0):
    """Fill device memory with synthetic frames (bench/test input utility)."""
    _check(lib().lm_synth_frames_device(device, C.c_void_p(d_ptr), rows, cols, first, n, pitch))


def match_cdf(image):
    """The cumulative histogram [256] float32 of a u8 image [rows, cols]
    (lm_match_cdf, include/locomouse_match.h; host only)."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 2:
        raise ValueError("image must be a 2-D uint8 array")
    image = np.ascontiguousarray(image)
    out = np.zeros(256, np.float32)
    _check(lib().lm_match_cdf(image.ctypes.data, image.shape[0], image.shape[1], image.shape[1], out.ctypes.data))
    return out


class Context:
    """One lm_ctx on one HIP device (the per-frame loop's state)."""

    def __init__(self, cfg, max_batch=64, device=0, lanes=None, reference_cdf=None):
        """lanes: pipeline lanes (lm_setup.pipeline_lanes; None keeps cfg.setup's).
        reference_cdf: [256] float32 (match_cdf of a reference image): a matched
        context, every frame's bottom crop matched to that histogram
        (lm_ctx_create_matched)."""
        self.cfg = cfg  # keeps the arrays behind the structs alive
        self._h = C.c_void_p()
        setup = cfg.setup
        if lanes is not None:
            setup = type(cfg.setup).from_buffer_copy(cfg.setup)
            setup.pipeline_lanes = lanes
        self._setup = setup
        if reference_cdf is not None:
            ref = np.ascontiguousarray(reference_cdf, dtype=np.float32)
            if ref.shape != (256,):
                raise ValueError("reference_cdf must hold 256 floats")
            _check(lib().lm_ctx_create_matched(device, C.byref(setup), C.byref(cfg.params), C.byref(cfg.model),
                                               ref.ctypes.data, max_batch, C.byref(self._h)))
        else:
            _check(lib().lm_ctx_create(device, C.byref(setup), C.byref(cfg.params), C.byref(cfg.model), max_batch,
                                       C.byref(self._h)))
        self.max_batch = max_batch

    def lanes(self):
        return lib().lm_ctx_lanes(self._h)

    def pending(self):
        return lib().lm_ctx_pending(self._h)

    def submit(self, frames, first_frame, prev_frame=None, bb=None):
        """Pipelined lm_detect_submit of host frames [n, rows, cols] u8."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        pp = None if prev_frame is None else np.ascontiguousarray(prev_frame, dtype=np.uint8)
        bbp = None if bb is None else np.ascontiguousarray(bb, dtype=np.int32)
        _check(lib().lm_detect_submit(self._h, frames.ctypes.data, frames.shape[1] * frames.shape[2], frames.shape[0],
                                      first_frame, None if pp is None else pp.ctypes.data,
                                      None if bbp is None else bbp.ctypes.data))

    def submit_device(self, d_frames_ptr, pitch, n, first_frame, d_prev_ptr=None, bb=None):
        """Pipelined lm_detect_submit_device (frames stay in device memory until collected)."""
        bbp = None if bb is None else np.ascontiguousarray(bb, dtype=np.int32)
        _check(lib().lm_detect_submit_device(self._h, C.c_void_p(d_frames_ptr), pitch, n, first_frame,
                                             C.c_void_p(d_prev_ptr) if d_prev_ptr else None,
                                             None if bbp is None else bbp.ctypes.data))

    def collect(self, raw=False):
        """Results of the oldest submitted batch (lm_detect_collect)."""
        res = lm_batch_result()
        _check(lib().lm_detect_collect(self._h, C.byref(res)))
        return res if raw else result_to_numpy(res)

    def geometry(self):
        g = lm_geometry()
        _check(lib().lm_get_geometry(self._h, C.byref(g)))
        return g

    def stream(self):
        return lib().lm_ctx_stream(self._h)

    def set_debug(self, flags):
        _check(lib().lm_ctx_set_debug(self._h, flags))

    def detect(self, frames, first_frame, prev_frame=None, bb=None, raw=False):
        """Host frames [n, rows, cols] u8 -> result dict (abi.result_to_numpy)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        res = lm_batch_result()
        pp = None
        if prev_frame is not None:
            self._prev = np.ascontiguousarray(prev_frame, dtype=np.uint8)
            pp = self._prev.ctypes.data
        bbp = None
        if bb is not None:
            self._bb = np.ascontiguousarray(bb, dtype=np.int32)
            bbp = self._bb.ctypes.data
        _check(lib().lm_detect_batch(self._h, frames.ctypes.data, frames.shape[1] * frames.shape[2], n, first_frame,
                                     pp, bbp, C.byref(res)))
        return res if raw else result_to_numpy(res)

    def detect_host_ptr(self, h_frames_ptr, pitch, n, first_frame, h_prev_ptr=None, raw=True):
        """lm_detect_batch on frames at a host address (e.g. a pinned torch
        tensor's data_ptr()): the H2D copy is part of the call."""
        res = lm_batch_result()
        _check(lib().lm_detect_batch(self._h, C.c_void_p(h_frames_ptr), pitch, n, first_frame,
                                     C.c_void_p(h_prev_ptr) if h_prev_ptr else None, None, C.byref(res)))
        return res if raw else result_to_numpy(res)

    def submit_host_ptr(self, h_frames_ptr, pitch, n, first_frame, h_prev_ptr=None):
        """Pipelined lm_detect_submit of frames at a host address (copied to
        the device before it returns)."""
        _check(lib().lm_detect_submit(self._h, C.c_void_p(h_frames_ptr), pitch, n, first_frame,
                                      C.c_void_p(h_prev_ptr) if h_prev_ptr else None, None))

    def detect_device(self, d_frames_ptr, pitch, n, first_frame, d_prev_ptr=None, bb=None, raw=True):
        """Frames already in device memory (e.g. a torch.cuda uint8 tensor's data_ptr())."""
        res = lm_batch_result()
        bbp = None
        if bb is not None:
            self._bb = np.ascontiguousarray(bb, dtype=np.int32)
            bbp = self._bb.ctypes.data
        _check(lib().lm_detect_batch_device(self._h, C.c_void_p(d_frames_ptr), pitch, n, first_frame,
                                            C.c_void_p(d_prev_ptr) if d_prev_ptr else None, bbp, C.byref(res)))
        return res if raw else result_to_numpy(res)

    def debug_scores(self, f, det):
        g = self.geometry()
        shapes = {0: (g.bb_bottom_mouse.height, g.bb_bottom_mouse.width), 1: (g.bb_bottom_mouse.height, g.bb_bottom_mouse.width),
                  2: (g.bb_bottom_mouse.height, g.tail_box_width), 3: (g.bb_side_mouse.height, g.bb_side_mouse.width),
                  4: (g.bb_side_mouse.height, g.bb_side_mouse.width), 5: (g.bb_side_mouse.height, g.tail_box_width)}
        out = np.zeros(shapes[det], dtype=np.float32)
        _check(lib().lm_debug_scores(self._h, f, det, out.ctypes.data, out.shape[0], out.shape[1]))
        return out

    def debug_tail_mask(self, f):
        g = self.geometry()
        out = np.zeros((g.bb_bottom_mouse.height, g.tail_box_width), dtype=np.uint8)
        _check(lib().lm_debug_tail_mask(self._h, f, out.ctypes.data, out.shape[0], out.shape[1]))
        return out

    def match_hist(self, f):
        """[256] uint32: the histogram of frame f's bottom crop in the last batch (lm_debug_match_hist)."""
        out = np.zeros(256, np.uint32)
        _check(lib().lm_debug_match_hist(self._h, f, out.ctypes.data))
        return out

    def match_table(self, f):
        """[256] uint8: frame f's table in the last batch (lm_debug_match_table)."""
        out = np.zeros(256, np.uint8)
        _check(lib().lm_debug_match_table(self._h, f, out.ctypes.data))
        return out

    def match_crop(self, f, prev=False):
        """The bottom box as frame f's steps see it: the current image, or
        (prev) I_PREV_PAD at the current box (lm_debug_match_crop; debug bit 1)."""
        g = self.geometry()
        out = np.zeros((g.bb_bottom_mouse.height, g.bb_bottom_mouse.width), np.uint8)
        _check(lib().lm_debug_match_crop(self._h, f, 1 if prev else 0, out.ctypes.data, out.shape[0], out.shape[1]))
        return out

    def kernel_times(self):
        names = (C.c_char_p * 64)()
        ms = (C.c_double * 64)()
        n = lib().lm_debug_kernel_times(self._h, names, ms, 64)
        return [(names[i].decode(), ms[i]) for i in range(min(n, 64))]

    def kernel_spans(self):
        """[(name, t0_ms, t1_ms)] of the last batch against the device epoch."""
        names = (C.c_char_p * 64)()
        t0 = (C.c_double * 64)()
        t1 = (C.c_double * 64)()
        n = lib().lm_debug_kernel_spans(self._h, names, t0, t1, 64)
        return [(names[i].decode(), t0[i], t1[i]) for i in range(min(n, 64))]

    def corr_work(self):
        """Bright (computed) output tiles and their consumed outputs of the last
        batch, bottom and side point detectors (lm_debug_corr_work), or None."""
        out = (C.c_int32 * 4)()
        _check(lib().lm_debug_corr_work(self._h, out))
        return None if out[0] < 0 else {"tiles": (out[0], out[1]), "outputs": (out[2], out[3])}

    def tail_work(self):
        """Tail tiles listed for computing and all tail tiles of the last
        batch, per tail detector (lm_debug_tail_work), or None with the skip
        off."""
        out = (C.c_int32 * 4)()
        _check(lib().lm_debug_tail_work(self._h, out))
        return None if out[0] < 0 else {"listed": (out[0], out[2]), "total": (out[1], out[3])}

    def screen_fallback(self):
        """Block sums of the tile-bound refinement that the fp32 screen left
        undecided and the double sum settled, over every batch of this context
        so far (lm_debug_screen_fallback); 0 with LM_TILE_SCREEN=0."""
        out = C.c_int64(0)
        _check(lib().lm_debug_screen_fallback(self._h, C.byref(out)))
        return int(out.value)

    def narrow_work(self):
        """{detector id: (narrow, wide)} tiles of the last batch's ring work
        (lm_debug_narrow_work); None where the narrow class is off."""
        out = (C.c_int32 * 12)()
        _check(lib().lm_debug_narrow_work(self._h, out))
        if all(out[k] < 0 for k in range(12)):
            return None
        return {d: (out[2 * d], out[2 * d + 1]) for d in range(6) if out[2 * d] >= 0}

    def narrow_entries(self, det, narrow, cap=None):
        """u64 entries of detector det's narrow (or wide) list of the last
        batch (lm_debug_narrow_entries): slot << 16 | tile in the low word,
        first block | count << 4 in the high word of a narrow one."""
        if cap is None:  # the list's own count
            cap = max(1, (self.narrow_work() or {}).get(det, (0, 0))[0 if narrow else 1])
        out = np.zeros(cap, np.uint64)
        n = C.c_int32(0)
        _check(lib().lm_debug_narrow_entries(self._h, det, 1 if narrow else 0, out.ctypes.data, cap, C.byref(n)))
        return out[:n.value].copy()

    def tail_tiles(self, f, view):
        """[tile rows, tile columns] u8: 1 where frame f's tile of tail
        detector `view` (0 bottom, 1 side) was listed (lm_debug_tail_tiles)."""
        g = self.geometry()
        tw, th = self.dark_tile_shape()
        oh = (g.bb_side_mouse if view else g.bb_bottom_mouse).height
        out = np.zeros((-(-oh // th), -(-g.tail_box_width // tw)), dtype=np.uint8)
        _check(lib().lm_debug_tail_tiles(self._h, f, view, out.ctypes.data, out.shape[0], out.shape[1]))
        return out

    def point_work(self):
        """Tiles listed for computing and bright tiles of the last batch, for
        paw_bottom, snout_bottom, paw_side, snout_side (lm_debug_point_work),
        or None with the skip off."""
        out = (C.c_int32 * 8)()
        _check(lib().lm_debug_point_work(self._h, out))
        return None if out[0] < 0 else {"listed": tuple(out[0:8:2]), "bright": tuple(out[1:8:2])}

    def point_tiles(self, f, det):
        """[tile rows, tile columns] u8: 1 where frame f's tile of point
        detector `det` (0 paw_bottom, 1 snout_bottom, 3 paw_side, 4
        snout_side) was listed (lm_debug_point_tiles)."""
        g = self.geometry()
        tw, th = self.dark_tile_shape()
        box = g.bb_side_mouse if det >= 3 else g.bb_bottom_mouse
        out = np.zeros((-(-box.height // th), -(-box.width // tw)), dtype=np.uint8)
        _check(lib().lm_debug_point_tiles(self._h, f, det, out.ctypes.data, out.shape[0], out.shape[1]))
        return out

    def batch_slots(self):
        """Frame slots the last collected batch processed (n, or n + 1 with
        its halo frame recomputed; lm_debug_batch_slots)."""
        return lib().lm_debug_batch_slots(self._h)

    @staticmethod
    def dark_tile_shape():
        """(columns, rows) of the dark-tile grid's tiles
        (lm_debug_dark_tile_width / _height)."""
        L = lib()  # (bound here, not at load: A/B runs load older libraries)
        return int(L.lm_debug_dark_tile_width()), int(L.lm_debug_dark_tile_height())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BBContext:
    """One lm_bb_ctx: the whole-video bounding-box pass (method 0,
    LocoMouse::computeBoundingBox, LocoMouse_class.cpp:579-653) on one HIP
    device.  Frames are pushed in video order; finish() post-processes."""

    def __init__(self, setup, bb_params, max_batch=64, device=0):
        self._setup, self._params = setup, bb_params  # keep the structs alive
        self._h = C.c_void_p()
        _check(lib().lm_bb_create(device, C.byref(setup), C.byref(bb_params), max_batch, C.byref(self._h)))
        self.max_batch = max_batch
        self.rows, self.cols = setup.calib_rows, setup.calib_cols

    def push(self, frames):
        """Host frames [n, rows, cols] u8 -> per-frame values (BB_FRAME_DTYPE)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        out = np.zeros(frames.shape[0], dtype=BB_FRAME_DTYPE)
        _check(lib().lm_bb_push(self._h, frames.ctypes.data, frames.shape[1] * frames.shape[2], frames.shape[0],
                                out.ctypes.data))
        return out

    def push_device(self, d_frames_ptr, pitch, n, values=True):
        out = np.zeros(n, dtype=BB_FRAME_DTYPE) if values else None
        _check(lib().lm_bb_push_device(self._h, C.c_void_p(d_frames_ptr), pitch, n,
                                       out.ctypes.data if values else None))
        return out

    def finish(self):
        r = lm_bb_result()
        _check(lib().lm_bb_finish(self._h, C.byref(r)))
        n = r.n_frames

        def arr(ptr, dtype):
            return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype).copy()
        per = np.frombuffer(C.cast(r.frames, C.POINTER(C.c_uint8 * (n * BB_FRAME_DTYPE.itemsize))).contents,
                            dtype=BB_FRAME_DTYPE, count=n).copy()
        return {"frames": per, "x_pos": arr(r.x_pos, np.uint32), "y_bottom_pos": arr(r.y_bottom_pos, np.uint32),
                "y_side_pos": arr(r.y_side_pos, np.uint32), "bb_side_mouse": r.bb_side_mouse.tuple(),
                "bb_bottom_mouse": r.bb_bottom_mouse.tuple()}

    def debug_binary(self, f):
        out = np.zeros((self.rows, self.cols), dtype=np.uint8)
        _check(lib().lm_bb_debug_binary(self._h, f, out.ctypes.data, self.rows, self.cols))
        return out

    def stream(self):
        return lib().lm_bb_stream(self._h)

    @staticmethod
    def dark_tile_shape():
        """(columns, rows) of the dark-tile grid's tiles
        (lm_debug_dark_tile_width / _height)."""
        L = lib()  # (bound here, not at load: A/B runs load older libraries)
        return int(L.lm_debug_dark_tile_width()), int(L.lm_debug_dark_tile_height())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_bb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def jpeg_probe(data):
    """lm_jpeg_probe: what a JPEG frame is (host only, no GPU call) as a dict;
    status is abi.LM_JPEG_OK when the device decoder takes it."""
    info = lm_jpeg_info()
    _check(lib().lm_jpeg_probe(bytes(data), len(data), C.byref(info)))
    d = {n: getattr(info, n) for n, _ in lm_jpeg_info._fields_ if n not in ("reserved", "reason")}
    d["reason"] = info.reason.decode()
    return d


class JpegDecoder:
    """One lm_jpeg_ctx: JPEG frames of rows x cols decoded on one HIP device
    from their compressed bytes (include/locomouse_jpeg.h)."""

    def __init__(self, rows, cols, max_batch=64, device=0, subseq_bytes=0):
        self._h = C.c_void_p()
        _check(lib().lm_jpeg_create(device, rows, cols, max_batch, subseq_bytes, C.byref(self._h)))
        self.rows, self.cols, self.max_batch, self.device = rows, cols, max_batch, device

    probe = staticmethod(jpeg_probe)

    def decode_into(self, jpegs, d_out_ptr, pitch=None):
        """lm_jpeg_decode_device into device memory at d_out_ptr (frame i at
        d_out_ptr + i * pitch); returns the per-frame statuses (int32 array)."""
        n = len(jpegs)
        keep = [bytes(j) for j in jpegs]
        ptrs = (C.c_char_p * max(n, 1))(*keep)
        sizes = (C.c_size_t * max(n, 1))(*[len(j) for j in keep])
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib().lm_jpeg_decode_device(self._h, ptrs, sizes, n, C.c_void_p(d_out_ptr),
                                           self.rows * self.cols if pitch is None else pitch,
                                           status.ctypes.data_as(C.POINTER(C.c_int32))))
        return status[:n]

    def decode(self, jpegs):
        """Frames as a torch uint8 tensor [n, rows, cols] on the decoder's
        device, and the per-frame statuses."""
        import torch
        out = torch.empty((max(len(jpegs), 1), self.rows, self.cols), dtype=torch.uint8, device=f"cuda:{self.device}")
        torch.cuda.synchronize(self.device)  # (the decode runs on the context's own stream)
        status = self.decode_into(jpegs, out.data_ptr())
        return out[:len(jpegs)], status

    def stats(self):
        s = lm_jpeg_stats()
        _check(lib().lm_jpeg_debug_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in lm_jpeg_stats._fields_}

    def set_interval_path(self, on):
        """lm_jpeg_set_interval_path: restart-interval frames one lane per interval (the default), or every frame
        through the subsequence path."""
        _check(lib().lm_jpeg_set_interval_path(self._h, int(bool(on))))

    def interval_stats(self):
        s = lm_jpeg_interval_stats()
        _check(lib().lm_jpeg_debug_interval_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in lm_jpeg_interval_stats._fields_ if n != "reserved"}

    def stream(self):
        return lib().lm_jpeg_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_jpeg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BackgroundEstimator:
    """One lm_bkg_ctx: the video's background as the per-pixel temporal median
    (or another rank) of its frames, on one HIP device
    (include/locomouse_bkg.h).  finish() equals
    np.sort(stack, axis=0)[(permille * (K - 1)) // 1000] of the K pushed frames."""

    def __init__(self, rows, cols, max_batch=64, device=0):
        self._h = C.c_void_p()
        _check(lib().lm_bkg_create(device, rows, cols, max_batch, C.byref(self._h)))
        self.rows, self.cols, self.max_batch, self.device = rows, cols, max_batch, device

    def push(self, frames):
        """Host frames [n, rows, cols] u8."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3 or frames.shape[1:] != (self.rows, self.cols):
            raise ValueError(f"frames must be [n, {self.rows}, {self.cols}], not {frames.shape}")
        _check(lib().lm_bkg_push(self._h, frames.ctypes.data, self.rows * self.cols, frames.shape[0]))

    def push_device(self, d_frames_ptr, pitch, n):
        """Frames in device memory (frame i at d_frames_ptr + i * pitch); they
        must stay unchanged until the context's stream has passed the push."""
        _check(lib().lm_bkg_push_device(self._h, C.c_void_p(d_frames_ptr), pitch, n))

    def finish(self, permille=500):
        out = np.zeros((self.rows, self.cols), dtype=np.uint8)
        _check(lib().lm_bkg_finish(self._h, permille, out.ctypes.data))
        return out

    def reset(self):
        _check(lib().lm_bkg_reset(self._h))

    @property
    def samples(self):
        return int(lib().lm_bkg_samples(self._h))

    def stream(self):
        return lib().lm_bkg_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_bkg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def calib_opts(**kw):
    """lm_calib_opts: the defaults (lm_calib_default_opts) with the given fields replaced."""
    o = lm_calib_opts()
    lib().lm_calib_default_opts(C.byref(o))
    for k, v in kw.items():
        if k not in dict(lm_calib_opts._fields_):
            raise TypeError(f"lm_calib_opts has no field {k}")
        setattr(o, k, v)
    return o


def calib_fit(records, rows, cols, split_row, opts=None, degree=2, max_resid=1.5):
    """lm_calib_fit (no GPU call) of records [n_frames, 2] (CALIB_RECORD_DTYPE: side, bottom) as a dict; a refusal
    raises LMError with its text."""
    rec = np.ascontiguousarray(records, dtype=CALIB_RECORD_DTYPE).reshape(-1, 2)
    res = lm_calib_fit_result()
    _check(lib().lm_calib_fit(rec.ctypes.data if len(rec) else (lm_calib_record * 2)(), len(rec), rows, cols, split_row,
                              None if opts is None else C.byref(opts), degree, max_resid, C.byref(res)))
    d = {n: getattr(res, n) for n, _ in lm_calib_fit_result._fields_ if n != "coef"}
    d["coef"] = [res.coef[k] for k in range(degree + 1)]
    d["raw"] = res
    return d


def calib_map(fit, rows, cols, split_row):
    """lm_calib_map (no GPU call): (ind_warp_mapping [rows, cols] int32, view_boxes [2, 4] int32) of calib_fit's result."""
    m = np.zeros((rows, cols), np.int32)
    boxes = np.zeros((2, 4), np.int32)
    _check(lib().lm_calib_map(C.byref(fit["raw"]), rows, cols, split_row, m.ctypes.data, boxes.ctypes.data))
    return m, boxes


class Calibrator:
    """One lm_calib_ctx: the marker's record in both views (side: rows [0, split_row), bottom: the rest) of every
    pushed frame, on one HIP device (include/locomouse_calib.h).  records() are exact integers; calib_fit and
    calib_map turn them into the calibration map on the host."""

    def __init__(self, rows, cols, split_row, max_batch=64, device=0, opts=None):
        self._h = C.c_void_p()
        self.opts = opts
        _check(lib().lm_calib_create(device, rows, cols, split_row, max_batch, None if opts is None else C.byref(opts),
                                     C.byref(self._h)))
        self.rows, self.cols, self.split_row, self.max_batch, self.device = rows, cols, split_row, max_batch, device

    def set_background(self, image):
        """Host image [rows, cols] u8, subtracted from the frames pushed after this call."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.shape != (self.rows, self.cols):
            raise ValueError(f"the background must be [{self.rows}, {self.cols}], not {image.shape}")
        _check(lib().lm_calib_set_background(self._h, image.ctypes.data))

    def push(self, frames):
        """Host frames [n, rows, cols] u8."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim != 3 or frames.shape[1:] != (self.rows, self.cols):
            raise ValueError(f"frames must be [n, {self.rows}, {self.cols}], not {frames.shape}")
        _check(lib().lm_calib_push(self._h, frames.ctypes.data, self.rows * self.cols, frames.shape[0]))

    def push_device(self, d_frames_ptr, pitch, n):
        """Frames in device memory (frame i at d_frames_ptr + i * pitch); they must stay unchanged until the
        context's stream has passed the push."""
        _check(lib().lm_calib_push_device(self._h, C.c_void_p(d_frames_ptr), pitch, n))

    @property
    def frames(self):
        return int(lib().lm_calib_frames(self._h))

    def records(self, first=0, n=None):
        """[n, 2] CALIB_RECORD_DTYPE (side, bottom) of frames first .. first + n - 1; waits for the stream."""
        if n is None:
            n = self.frames - first
        out = np.zeros((max(n, 0), 2), dtype=CALIB_RECORD_DTYPE)
        _check(lib().lm_calib_read(self._h, first, n, out.ctypes.data if out.size else (lm_calib_record * 2)()))
        return out

    def reset(self):
        _check(lib().lm_calib_reset(self._h))

    def stream(self):
        return lib().lm_calib_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_calib_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Trainer:
    """One lm_train_ctx: kh x kw u8 patches with labels +1 / -1 on one HIP
    device, and the L2-regularised squared-hinge SVM solved on them in fp64
    (include/locomouse_train.h).  solve() returns the detector (W, rho) whose
    score sum(W * patch) - rho is the SVM's margin, and the solver's stats."""

    def __init__(self, kh, kw, max_samples, device=0):
        self._h = C.c_void_p()
        _check(lib().lm_train_create(device, kh, kw, max_samples, C.byref(self._h)))
        self.kh, self.kw, self.max_samples, self.device = kh, kw, max_samples, device

    def add_patches(self, patches, labels):
        """patches [n, kh, kw] or [n, kh * kw] u8, labels [n] of +1 / -1."""
        patches = np.ascontiguousarray(patches, dtype=np.uint8)
        labels = np.ascontiguousarray(labels, dtype=np.int8)
        n = labels.shape[0]
        if patches.size != n * self.kh * self.kw:
            raise ValueError(f"patches must hold {n} x {self.kh} x {self.kw} bytes, not {patches.shape}")
        _check(lib().lm_train_add_patches(self._h, patches.ctypes.data, labels.ctypes.data, n))

    @staticmethod
    def _points(points):
        pts = np.ascontiguousarray(points, dtype=np.int32).reshape(-1, 4)  # (frame, x, y, label)
        return pts, pts.ctypes.data if len(pts) else None

    def gather(self, ctx, frames, points):
        """One patch per point (frame, x, y, label), x and y in the corrected
        image, cut from host frames [n, rows, cols] u8 as the detection
        Context `ctx` reads them."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        pts, pp = self._points(points)
        _check(lib().lm_train_gather(self._h, ctx._h, frames.ctypes.data, frames.shape[1] * frames.shape[2],
                                     frames.shape[0], pp, len(pts)))

    def gather_device(self, ctx, d_frames_ptr, pitch, n_frames, points):
        """The same for frames in device memory (frame i at d_frames_ptr + i * pitch)."""
        pts, pp = self._points(points)
        _check(lib().lm_train_gather_device(self._h, ctx._h, C.c_void_p(d_frames_ptr), pitch, n_frames, pp, len(pts)))

    def samples(self):
        """(positives, negatives) stored."""
        a, b = C.c_int32(), C.c_int32()
        _check(lib().lm_train_samples(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def reset(self):
        _check(lib().lm_train_reset(self._h))

    def patches(self, first=0, n=None):
        """(patches [n, kh, kw] u8, labels [n] int8) as they are stored."""
        if n is None:
            n = sum(self.samples()) - first
        out = np.zeros((n, self.kh, self.kw), np.uint8)
        lab = np.zeros(n, np.int8)
        _check(lib().lm_train_patches(self._h, first, n, out.ctypes.data, lab.ctypes.data))
        return out, lab

    def solve(self, c_pos=10.0, c_neg=1.0, eps=1e-6, max_iter=100):
        """(W [kh, kw] float64, rho, stats dict)."""
        W = np.zeros((self.kh, self.kw), np.float64)
        rho = C.c_double()
        st = lm_train_stats()
        _check(lib().lm_train_solve(self._h, c_pos, c_neg, eps, max_iter, W.ctypes.data, C.byref(rho), C.byref(st)))
        return W, rho.value, {n: getattr(st, n) for n, _ in lm_train_stats._fields_}

    def set_groups(self, groups):
        """A group in 0..255 for every stored sample (the folds of a cross-validation);
        forgotten by the next add_patches, gather or reset."""
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        _check(lib().lm_train_set_groups(self._h, g.ctypes.data, len(g)))

    def problem_block(self):
        """Problems that share one pass over the sample matrix at this kh x kw."""
        return int(lib().lm_train_problem_block(self._h))

    def solve_many(self, problems, eps=1e-6, max_iter=100):
        """problems: [(c_pos, c_neg, held_out)], held_out a group or -1.  Returns
        (Ws, rhos, stats, heldout): per problem W [kh, kw] float64, rho, the
        stats dict and the held-out group's counts {n_pos, n_neg, miss_pos,
        miss_neg}, each problem's what it gets alone."""
        n = len(problems)
        pr = (lm_train_problem * max(n, 1))(*[lm_train_problem(float(a), float(b), int(h), 0) for a, b, h in problems])
        W = np.zeros((max(n, 1), self.kh, self.kw), np.float64)
        rho = np.zeros(max(n, 1), np.float64)
        st = (lm_train_stats * max(n, 1))()
        ho = (lm_train_heldout * max(n, 1))()
        _check(lib().lm_train_solve_many(self._h, C.addressof(pr), n, eps, max_iter, W.ctypes.data, rho.ctypes.data,
                                         C.addressof(st), C.addressof(ho)))
        return ([W[q].copy() for q in range(n)], [float(rho[q]) for q in range(n)],
                [{k: getattr(st[q], k) for k, _ in lm_train_stats._fields_} for q in range(n)],
                [{k: getattr(ho[q], k) for k, _ in lm_train_heldout._fields_} for q in range(n)])

    def margins(self, W, rho):
        """z_i = sum(W * patch_i) - rho of the stored samples."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.size != self.kh * self.kw:
            raise ValueError(f"W must hold {self.kh} x {self.kw} doubles, not {W.shape}")
        z = np.zeros(sum(self.samples()), np.float64)
        _check(lib().lm_train_margins(self._h, W.ctypes.data, float(rho), z.ctypes.data))
        return z

    def stream(self):
        return lib().lm_train_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_train_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JpegEncoder:
    """One lm_enc_ctx: frames of rows x cols (LM_ENC_GRAY8, or LM_ENC_RGB24 as
    YCbCr 4:2:0) encoded as baseline JPEG files on one HIP device, byte for
    byte the host encoder's and libjpeg's (include/locomouse_encode.h); with
    set_overlay(), raw frames rendered through the calibration map with marks
    drawn on them first.  restart_interval (in MCUs, 0: none) writes libjpeg's
    restart markers (lm_enc_create_restart)."""

    GRAY8, RGB24 = LM_ENC_GRAY8, LM_ENC_RGB24

    def __init__(self, rows, cols, fmt=LM_ENC_GRAY8, quality=90, max_batch=64, device=0, restart_interval=0):
        self._h = C.c_void_p()
        _check(lib().lm_enc_create_restart(device, rows, cols, fmt, quality, max_batch, restart_interval, C.byref(self._h)))
        self.rows, self.cols, self.fmt, self.quality = rows, cols, fmt, quality
        self.restart_interval = restart_interval
        self.max_batch, self.device = max_batch, device
        self.frame_bytes = rows * cols * (3 if fmt == LM_ENC_RGB24 else 1)
        self._src = None

    @staticmethod
    def slot_bytes(rows, cols, fmt, restart_interval=0):
        return int(lib().lm_enc_slot_bytes_restart(rows, cols, fmt, restart_interval))

    @staticmethod
    def _files(res):
        n = res.n
        total = res.offset[n - 1] + res.size[n - 1]
        data = C.string_at(res.data, total)
        return [data[res.offset[i]:res.offset[i] + res.size[i]] for i in range(n)]

    def encode(self, frames):
        """Host frames [n, rows, cols] (grey) or [n, rows, cols, 3] (RGB) u8 -> the n JPEG files (bytes)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        want = (self.rows, self.cols) if self.fmt == LM_ENC_GRAY8 else (self.rows, self.cols, 3)
        if frames.shape[1:] != want:
            raise ValueError(f"frames must be [n, {', '.join(map(str, want))}], not {frames.shape}")
        res = lm_enc_result()
        _check(lib().lm_enc_encode(self._h, frames.ctypes.data, self.frame_bytes, frames.shape[0], C.byref(res)))
        return self._files(res)

    def encode_device(self, d_frames_ptr, n, pitch=None, files=True):
        """Frames in device memory (frame i at d_frames_ptr + i * pitch)."""
        res = lm_enc_result()
        _check(lib().lm_enc_encode_device(self._h, C.c_void_p(d_frames_ptr), self.frame_bytes if pitch is None else pitch, n,
                                          C.byref(res)))
        return self._files(res) if files else None

    def set_overlay(self, cal, src_rows, src_cols, flip):
        """The canvas geometry: cal [rows, cols] int32 indices into a raw src_rows x src_cols frame."""
        self._cal = np.ascontiguousarray(cal, dtype=np.int32)
        geo = lm_enc_overlay(C.cast(self._cal.ctypes.data, C.POINTER(C.c_int32)), src_rows, src_cols, self._cal.shape[0],
                             self._cal.shape[1], int(bool(flip)), 0)
        _check(lib().lm_enc_set_overlay(self._h, C.byref(geo)))
        self._src = (src_rows, src_cols)

    @staticmethod
    def _marks(marks_per_frame):
        flat = [m for per in marks_per_frame for m in per]
        arr = (lm_enc_mark * max(len(flat), 1))(*[lm_enc_mark(*map(int, m)) for m in flat])
        off = np.zeros(len(marks_per_frame) + 1, np.int32)
        off[1:] = np.cumsum([len(per) for per in marks_per_frame])
        return arr, off

    def render_encode_device(self, d_raw_ptr, pitch, marks_per_frame, files=True):
        """Raw frames in device memory rendered with each frame's marks [(x, y, radius, colour), ...] and encoded."""
        arr, off = self._marks(marks_per_frame)
        res = lm_enc_result()
        _check(lib().lm_enc_render_encode_device(self._h, C.c_void_p(d_raw_ptr), pitch, len(marks_per_frame), arr,
                                                 off.ctypes.data, C.byref(res)))
        return self._files(res) if files else None

    def render_encode(self, raw, marks_per_frame):
        """The same for host frames [n, src_rows, src_cols] u8, uploaded first."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8)
        if raw.shape != (len(marks_per_frame), *self._src):
            raise ValueError(f"raw must be [{len(marks_per_frame)}, {self._src[0]}, {self._src[1]}], not {raw.shape}")
        arr, off = self._marks(marks_per_frame)
        res = lm_enc_result()
        _check(lib().lm_enc_render_encode(self._h, raw.ctypes.data, raw.shape[1] * raw.shape[2], raw.shape[0], arr,
                                          off.ctypes.data, C.byref(res)))
        return self._files(res)

    def render_device(self, d_raw_ptr, pitch, marks_per_frame):
        """The rendered canvases [n, rows, cols, 3] u8 (test access)."""
        arr, off = self._marks(marks_per_frame)
        out = np.zeros((len(marks_per_frame), self.rows, self.cols, 3), np.uint8)
        _check(lib().lm_enc_render_device(self._h, C.c_void_p(d_raw_ptr), pitch, len(marks_per_frame), arr, off.ctypes.data,
                                          out.ctypes.data))
        return out

    def stats(self):
        s = lm_enc_stats()
        _check(lib().lm_enc_last_stats(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in lm_enc_stats._fields_ if n != "reserved"}

    def stream(self):
        return lib().lm_enc_stream(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().lm_enc_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
