"""ctypes access to tests/cpp/enc_harness.cpp (the host JPEG encoder and the
MJPEG AVI writer), Pillow as the encoder's reference, and the images the
encoder tests share (CPU and GPU).  The harness links no GPU library."""
import ctypes as C
import functools
import io
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "locomouse_cpp_amd")
BUILD = os.path.join(HERE, "cpp", "_build")
SO = os.path.join(BUILD, "libenc_harness.so")
SRC = os.path.join(HERE, "cpp", "enc_harness.cpp")
INCLUDES = ["-I" + os.path.join(PKG, "host"), "-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include")]
HOST_SRCS = [os.path.join(PKG, "host", f) for f in ("JpegEncode.cpp", "Media.cpp", "Jpeg.cpp")]

GRAY8, RGB24 = 0, 1


def _deps():
    return [SRC, *HOST_SRCS, os.path.join(PKG, "host", "JpegEncode.hpp"), os.path.join(PKG, "host", "Media.hpp"),
            os.path.join(PKG, "csrc", "lm_jpeg_enc_core.h"), os.path.join(PKG, "csrc", "lm_jpeg_hdr.h")]


def build(verbose=False):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-pthread", *INCLUDES, "-o", SO, SRC, *HOST_SRCS, "-lz"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


_lib = None


def lib():
    """The harness, built on first use (and again when a source is newer)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in _deps()):
            build()
        L = C.CDLL(SO)
        L.eh_encode.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_char_p, C.c_int]
        L.eh_encode.restype = C.c_int64
        L.eh_coefficients.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
        L.eh_coefficients.restype = C.c_int64
        L.eh_encode_many.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
        L.eh_encode_many.restype = C.c_int64
        L.eh_write_avi.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_int,
                                   C.c_int]
        L.eh_avi_info.argtypes = [C.c_char_p, C.c_void_p]
        L.eh_avi_chunk.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int64]
        L.eh_avi_chunk.restype = C.c_int64
        L.eh_avi_frames.argtypes = [C.c_char_p, C.c_void_p, C.c_int]
        _lib = L
    return _lib


def fmt_of(img):
    return GRAY8 if img.ndim == 2 else RGB24


def slot_bytes(rows, cols, fmt):
    """The worst case of one file (include/locomouse_encode.h: lm_enc_slot_bytes)."""
    nblk = ((rows + 7) // 8) * ((cols + 7) // 8) if fmt == GRAY8 else 6 * ((rows + 15) // 16) * ((cols + 15) // 16)
    return 640 + 2 * (52 * 4 * nblk + 4) + 2


def host_encode(img, quality):
    """The host encoder's file for one image (H x W grey or H x W x 3 RGB, u8), or its error message (str)."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(slot_bytes(img.shape[0], img.shape[1], fmt_of(img)), np.uint8)
    err = C.create_string_buffer(256)
    n = lib().eh_encode(img.ctypes.data, img.shape[0], img.shape[1], fmt_of(img), quality, out.ctypes.data, out.size, err, 256)
    if n == -1:
        return err.value.decode()
    assert n >= 0, "the file passed its worst case"
    return out[:n].tobytes()


def host_coefficients(img, quality):
    """[blocks, 64] int16, scan order, zig-zag."""
    img = np.ascontiguousarray(img, np.uint8)
    out = np.zeros(slot_bytes(img.shape[0], img.shape[1], fmt_of(img)), np.int16)
    n = lib().eh_coefficients(img.ctypes.data, img.shape[0], img.shape[1], fmt_of(img), quality, out.ctypes.data, out.size)
    assert n >= 0
    return out[:n * 64].reshape(n, 64).copy()


def host_encode_many(frames, quality, threads):
    """The frames [n, H, W(, 3)] through the host encoder on `threads` threads; the files' total size."""
    frames = np.ascontiguousarray(frames, np.uint8)
    n = lib().eh_encode_many(frames.ctypes.data, frames.shape[1], frames.shape[2], fmt_of(frames[0]), quality, frames.shape[0],
                             threads)
    assert n >= 0
    return int(n)


def pillow_encode(img, quality):
    """Image.save(f, "JPEG", quality=q) for mode L; with subsampling=2 for mode RGB."""
    from PIL import Image
    b = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(np.ascontiguousarray(img, np.uint8), "L").save(b, "JPEG", quality=quality)
    else:
        Image.fromarray(np.ascontiguousarray(img, np.uint8), "RGB").save(b, "JPEG", quality=quality, subsampling=2)
    return b.getvalue()


def write_avi(path, jpegs, rows, cols, fps=30):
    keep = [bytes(j) for j in jpegs]
    ptrs = (C.c_char_p * max(len(keep), 1))(*keep)
    sizes = (C.c_size_t * max(len(keep), 1))(*[len(j) for j in keep])
    return lib().eh_write_avi(os.fsencode(path), ptrs, sizes, len(keep), rows, cols, fps)


def avi_info(path):
    info = np.zeros(5, np.int32)
    if lib().eh_avi_info(os.fsencode(path), info.ctypes.data):
        return None
    return dict(rows=int(info[0]), cols=int(info[1]), frames=int(info[2]), fps=int(info[3]), mjpeg=bool(info[4]))


def avi_chunks(path):
    """Every frame chunk's bytes, through AviReader::read_chunk."""
    info = avi_info(path)
    buf = np.zeros(slot_bytes(info["rows"], info["cols"], RGB24), np.uint8)
    out = []
    for i in range(info["frames"]):
        n = lib().eh_avi_chunk(os.fsencode(path), i, buf.ctypes.data, buf.size)
        assert n >= 0
        out.append(buf[:n].tobytes())
    return out


def avi_frames(path):
    """Every frame's channel 0, through AviReader::read."""
    info = avi_info(path)
    out = np.zeros((info["frames"], info["rows"], info["cols"]), np.uint8)
    n = lib().eh_avi_frames(os.fsencode(path), out.ctypes.data, info["frames"])
    return out[:max(n, 0)]


# ---- the images: explicit arrays, the same for the host and the device encoder
GREY_SIZES = ((8, 8), (16, 16), (17, 23), (24, 40), (8, 2048))
COLOUR_SIZES = ((8, 8), (9, 17), (16, 16), (17, 23), (24, 40), (33, 49))
QUALITIES = (1, 5, 25, 75, 90, 100)


def _seed(name, h, w):
    return sum(name.encode()) * 1000003 + h * 4099 + w


def grey_images(h, w):
    """name -> H x W u8."""
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(_seed("noise", h, w))
    smooth = 128 + 60 * np.sin(x / 9.0) * np.cos(y / 7.0)
    # one isolated high frequency (the (7, 7) cosine of each block) on a smooth image: long zero runs in front of it
    spike = smooth + 100 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    return {
        "noise": rng.integers(0, 256, size=(h, w)).astype(np.uint8),
        "const0": np.zeros((h, w), np.uint8),
        "const128": np.full((h, w), 128, np.uint8),
        "const255": np.full((h, w), 255, np.uint8),
        "checker": (((x + y) & 1) * 255).astype(np.uint8),
        "gradient": ((x * 255) // max(w - 1, 1) // 2 + (y * 255) // max(h - 1, 1) // 2).astype(np.uint8),
        "blocks": ((((x // 8) + (y // 8)) & 1) * 255).astype(np.uint8),
        "spike": np.clip(spike, 0, 255).astype(np.uint8),
    }


def colour_images(h, w):
    """name -> H x W x 3 u8 (R, G, B)."""
    out = {}
    rng = np.random.default_rng(_seed("rgbnoise", h, w))
    out["noise"] = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
    for name, g in grey_images(h, w).items():
        if name in ("const0", "const128", "const255", "checker", "gradient", "blocks", "spike"):
            out[name] = np.repeat(g[:, :, None], 3, axis=2)
    marked = np.repeat(grey_images(h, w)["gradient"][:, :, None], 3, axis=2).copy()
    palette = ((255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255), (0, 255, 255))
    for k, col in enumerate(palette):  # squares of side 3, some cut by the borders
        cy, cx = (k * 7) % h, (k * 11 + 3) % w
        marked[max(cy - 1, 0):cy + 2, max(cx - 1, 0):cx + 2] = col
    out["marks"] = marked
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """((name, image, quality), ...): every size x image x quality the issue lists.  The 'spike' image only at low
    quality (its point is the zero run a coarse table leaves in front of one coefficient)."""
    out = []
    for sizes, make, tag in ((GREY_SIZES, grey_images, "grey"), (COLOUR_SIZES, colour_images, "rgb")):
        for h, w in sizes:
            for name, img in make(h, w).items():
                for q in QUALITIES:
                    if name == "spike" and q > 25:
                        continue
                    img.setflags(write=False)
                    out.append((f"{tag}_{h}x{w}_{name}_q{q}", img, q))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pillow_files():
    """Pillow's file of every case, computed once."""
    return tuple(pillow_encode(img, q) for _, img, q in cases())


ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])  # zig-zag position -> natural index (T.81 figure A.6)
