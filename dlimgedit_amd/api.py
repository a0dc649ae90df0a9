"""Python host binding over the C-ABI of libdlimgedit.so (ctypes, no torch types anywhere).

Mirrors the reference's header-only C++ wrapper (reference: src/include/dlimgedit/dlimgedit.hpp and
detail/dlimgedit.impl.hpp): same class and method names, same argument meaning, errors surface as
`Error(last_error())` exactly where the C++ wrapper throws `dlimg::Exception`.  Only the slots of
`dlimg_Api` are used for the drop-in surface; the `ext` namespace exposes the extension entry points
of include/dlimgedit/dlimgedit_amd.h for benchmarks and parity tests.

The library is the product: if it is missing or the GPU is absent, calls fail loudly; there is no
fallback implementation in Python.
"""
from __future__ import annotations

import ctypes as C
import os
import enum
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Sequence, Tuple

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "lib" / "libdlimgedit.so"
# The test and benchmark hooks (include/dlimgedit/dlimgedit_amd_test.h: ext.test_*, ext.bench_*, ext.force_gemm_tile,
# ext.mask_pieces, ext.plan_steps) are not in the product library: they come from lib/libdlimgedit_test.so, the product's own
# objects plus the hook sources csrc/*test_hooks.cpp, loaded next to the product the first time a hook is called.
HOOKS_LIB_PATH = LIB_PATH.with_name("libdlimgedit_test.so")
# ext.test_matte and ext.test_stroke_derive come from a library of their own (build.py: LIB_MATTE_HOOKS; the tuning library has it as well)
MATTE_HOOKS_LIB_PATH = LIB_PATH.with_name("libdlimgedit_matte_hooks.so")
# tools/ only: the -DDLIMG_TUNING build with ablated kernel variants and in-kernel stamps (python -m dlimgedit_amd.build --tuning);
# it exports the hooks too, so one library serves both roles
if os.environ.get("DLIMGEDIT_TUNING_LIB") == "1":
    LIB_PATH = HOOKS_LIB_PATH = LIB_PATH.with_name("libdlimgedit_tuning.so")
elif os.environ.get("DLIMGEDIT_TUNING_LIB"):          # a copy of a tuning build kept under another name (A/B of several variants)
    LIB_PATH = HOOKS_LIB_PATH = LIB_PATH.with_name(os.environ["DLIMGEDIT_TUNING_LIB"])


class Error(RuntimeError):
    """dlimg::Exception."""


class Backend(enum.IntEnum):
    cpu = 0
    gpu = 1


class Channels(enum.IntEnum):
    mask = 1
    rgb = 3
    rgba = 4
    bgra = 5
    argb = 6


def count(channels: Channels) -> int:
    return 4 if int(channels) > 4 else int(channels)


@dataclass(frozen=True)
class Extent:
    width: int = 0
    height: int = 0


@dataclass(frozen=True)
class Point:
    x: int = 0
    y: int = 0


@dataclass(frozen=True)
class Region:
    top_left: Point = Point()
    bottom_right: Point = Point()

    @staticmethod
    def from_origin(origin: Point, extent: Extent) -> "Region":
        return Region(origin, Point(origin.x + extent.width, origin.y + extent.height))


# ---------------------------------------------------------------------------------------------
# C structs (layouts: include/dlimgedit/dlimgedit.h)

class _ImageView(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("channels", C.c_int), ("stride", C.c_int),
                ("pixels", C.c_void_p)]


class _Options(C.Structure):
    _fields_ = [("backend", C.c_int), ("model_directory", C.c_char_p)]


_u8pp = C.POINTER(C.c_void_p)

_API_FIELDS = [
    ("is_backend_supported", C.CFUNCTYPE(C.c_int, C.c_int)),
    ("create_environment", C.CFUNCTYPE(C.c_int, C.POINTER(C.c_void_p), C.POINTER(_Options))),
    ("destroy_environment", C.CFUNCTYPE(None, C.c_void_p)),
    ("process_image_for_segmentation", C.CFUNCTYPE(C.c_int, C.POINTER(C.c_void_p), C.POINTER(_ImageView), C.c_void_p)),
    ("get_segmentation_mask", C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _u8pp,
                                          C.POINTER(C.c_float))),
    ("get_segmentation_extent", C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_int))),
    ("destroy_segmentation", C.CFUNCTYPE(None, C.c_void_p)),
    ("segment_objects", C.CFUNCTYPE(C.c_int, C.POINTER(_ImageView), C.c_void_p, C.c_void_p)),
    ("load_image", C.CFUNCTYPE(C.c_int, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), _u8pp)),
    ("save_image", C.CFUNCTYPE(C.c_int, C.POINTER(_ImageView), C.c_char_p)),
    ("create_image", C.CFUNCTYPE(C.c_void_p, C.c_int, C.c_int, C.c_int)),
    ("destroy_image", C.CFUNCTYPE(None, C.c_void_p)),
    ("last_error", C.CFUNCTYPE(C.c_char_p)),
    # additions of this build
    ("process_images_for_segmentation", C.CFUNCTYPE(C.c_int, C.POINTER(C.c_void_p), C.POINTER(_ImageView), C.c_int,
                                                    C.c_void_p)),
    ("get_segmentation_masks", C.CFUNCTYPE(C.c_int, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int),
                                           C.POINTER(C.c_int), _u8pp)),
]

REFERENCE_SLOTS = 13     # the reference's table ends after last_error


class _Api(C.Structure):
    _fields_ = _API_FIELDS


_lib = None
_api = None


def library() -> C.CDLL:
    """Loads libdlimgedit.so; raises if it has not been built (`python -m dlimgedit_amd.build`)."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise Error(f"{LIB_PATH} not found: build it with `python -m dlimgedit_amd.build` "
                        "(the HIP library is the product; there is no Python fallback)")
        _lib = C.CDLL(str(LIB_PATH))
        _lib.dlimg_init.restype = C.POINTER(_Api)
        _lib.dlimg_init.argtypes = []
    return _lib


_hooks_lib = None


def hooks_library() -> C.CDLL:
    """Loads the library that exports the test / benchmark hooks (libdlimgedit_test.so; the tuning library when one is
    selected).  Raises if it has not been built: there is no fallback, a hook never runs anything but HIP code."""
    global _hooks_lib
    if _hooks_lib is None:
        if HOOKS_LIB_PATH == LIB_PATH:
            _hooks_lib = library()
        else:
            if not HOOKS_LIB_PATH.exists():
                raise Error(f"{HOOKS_LIB_PATH} not found: build it with `python -m dlimgedit_amd.build`")
            _hooks_lib = C.CDLL(str(HOOKS_LIB_PATH))
            _hooks_lib.dlimg_init.restype = C.POINTER(_Api)
            _hooks_lib.dlimg_init.argtypes = []
    return _hooks_lib


_matte_hooks_lib = None


def matte_hooks_library() -> C.CDLL:
    """Loads the library that exports dlimg_amd_test_matte and dlimg_amd_test_stroke_derive (libdlimgedit_matte_hooks.so; the
    tuning library when one is selected).  Raises if it has not been built."""
    global _matte_hooks_lib
    if _matte_hooks_lib is None:
        if HOOKS_LIB_PATH == LIB_PATH:
            _matte_hooks_lib = library()
        else:
            if not MATTE_HOOKS_LIB_PATH.exists():
                raise Error(f"{MATTE_HOOKS_LIB_PATH} not found: build it with `python -m dlimgedit_amd.build`")
            _matte_hooks_lib = C.CDLL(str(MATTE_HOOKS_LIB_PATH))
            _matte_hooks_lib.dlimg_init.restype = C.POINTER(_Api)
            _matte_hooks_lib.dlimg_init.argtypes = []
        _ip, _vpp = C.POINTER(C.c_int), C.POINTER(C.c_void_p)
        _matte_hooks_lib.dlimg_amd_test_matte.argtypes = [_vpp, _vpp, _ip, _ip, _ip, _ip, _ip, C.c_int, C.c_int, _ip, _ip, C.c_int,
                                                          C.POINTER(C.c_float)]
        _matte_hooks_lib.dlimg_amd_test_matte.restype = C.c_int
        _matte_hooks_lib.dlimg_amd_test_stroke_derive.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32),
                                                                  C.POINTER(C.c_uint64), _ip, C.c_int, C.POINTER(C.c_float)]
        _matte_hooks_lib.dlimg_amd_test_stroke_derive.restype = C.c_int
        _matte_hooks_lib.dlimg_amd_test_cutout.argtypes = [_vpp, _vpp, _vpp, _ip, _ip, _ip, _ip, C.c_int, C.c_int, _ip, _ip, C.c_int,
                                                           C.POINTER(C.c_float)]
        _matte_hooks_lib.dlimg_amd_test_cutout.restype = C.c_int
        _matte_hooks_lib.dlimg_amd_test_edge.argtypes = [_vpp, _ip, _ip, _ip, _ip, _ip, C.c_int, C.c_int, _ip, _ip, C.c_int,
                                                         C.POINTER(C.c_float)]
        _matte_hooks_lib.dlimg_amd_test_edge.restype = C.c_int
    return _matte_hooks_lib


def _check_hook(result: int) -> None:
    """As _check, with the message of the library the hook lives in (last_error is per library and per thread)."""
    if result != 0:
        msg = hooks_library().dlimg_init().contents.last_error()
        raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")


def api() -> _Api:
    """dlimg::api(): the function table, initialised on first use (handle.hpp:27-34 in the reference)."""
    global _api
    if _api is None:
        _api = library().dlimg_init().contents
    return _api


def _check(result: int) -> None:
    if result != 0:
        msg = api().last_error()
        raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")


# ---------------------------------------------------------------------------------------------
# Image / ImageView

class ImageView:
    """Non-owning view of u8 pixels (numpy array kept alive by the view)."""

    def __init__(self, pixels: np.ndarray, channels: Channels = Channels.rgba, stride: Optional[int] = None):
        if pixels.dtype != np.uint8:
            raise TypeError("pixels must be uint8")
        if pixels.ndim == 2:
            pixels = pixels[:, :, None]
        h, w, c = pixels.shape
        if c != count(channels):
            raise ValueError(f"array has {c} channels, {channels!r} needs {count(channels)}")
        if stride is None:
            pixels = np.ascontiguousarray(pixels)
            stride = w * c
        self._array = pixels
        self.extent = Extent(w, h)
        self.channels = Channels(channels)
        self.stride = int(stride)

    def _c(self) -> _ImageView:
        return _ImageView(self.extent.width, self.extent.height, int(self.channels), self.stride,
                          self._array.ctypes.data)


class Image:
    """Owning image allocated by the library (create_image / destroy_image)."""

    def __init__(self, extent: Extent, channels: Channels = Channels.rgba):
        self._extent, self._channels = extent, Channels(channels)
        self._ptr = api().create_image(extent.width, extent.height, count(channels))
        if not self._ptr:
            raise Error("create_image failed")

    def extent(self) -> Extent:
        return self._extent

    def channels(self) -> Channels:
        return self._channels

    def size(self) -> int:
        return self._extent.width * self._extent.height * count(self._channels)

    def pixels(self) -> np.ndarray:
        buf = (C.c_uint8 * self.size()).from_address(self._ptr)
        buf._owner = self                        # the array keeps the Image (and with it the library's allocation) alive
        return np.frombuffer(buf, dtype=np.uint8).reshape(self._extent.height, self._extent.width, count(self._channels))

    def view(self) -> ImageView:
        return ImageView(self.pixels(), self._channels)

    @staticmethod
    def load(filepath) -> "Image":
        ext = (C.c_int * 2)()
        ch = C.c_int()
        px = C.c_void_p()
        _check(api().load_image(str(filepath).encode(), ext, C.byref(ch), C.byref(px)))
        img = Image.__new__(Image)               # adopt the library's allocation (freed by destroy_image)
        img._extent, img._channels, img._ptr = Extent(ext[0], ext[1]), Channels(ch.value), px.value
        return img

    @staticmethod
    def save(img: ImageView, filepath) -> None:
        v = img._c()
        _check(api().save_image(C.byref(v), str(filepath).encode()))

    def __del__(self):
        ptr, self._ptr = getattr(self, "_ptr", None), None
        if ptr and _api is not None:
            _api.destroy_image(ptr)


def _mask_image(extent: Extent) -> np.ndarray:
    """A result mask as the reference's wrapper makes it -- `Image(extent(), Channels::mask)`, i.e. memory from the library's
    create_image (dlimgedit.impl.hpp:84-88) -- seen as an (h, w) array that keeps the Image alive."""
    return Image(extent, Channels.mask).pixels().reshape(extent.height, extent.width)


# ---------------------------------------------------------------------------------------------
# Environment / Segmentation

@dataclass
class Options:
    backend: Backend = Backend.cpu
    model_directory: str = "models"


class Environment:
    """dlimg::Environment: owns the model cache; must outlive every Segmentation made from it."""

    @staticmethod
    def is_supported(backend: Backend) -> bool:
        return api().is_backend_supported(int(backend)) != 0

    def __init__(self, options: Options = Options()):
        self._handle = C.c_void_p()
        self._dir = str(options.model_directory).encode()
        opts = _Options(int(options.backend), self._dir)
        _check(api().create_environment(C.byref(self._handle), C.byref(opts)))

    def handle(self) -> C.c_void_p:
        return self._handle

    def close(self) -> None:
        h, self._handle = self._handle, C.c_void_p()
        if h and _api is not None:
            _api.destroy_environment(h)

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@dataclass
class Mask:
    image: np.ndarray        # [H, W] uint8, values 0 or 255
    accuracy: float = 0.0


MAX_CLICKS = 8               # clicks of one prompt (csrc/prompt_plan.hpp: kMaxClicks)
TOKEN_ROWS_MAX = 112         # token rows of one decoder launch (csrc/kernels/kernels.hpp: kDecoderMaxRows)
EMPTY_REGION = (0, 0, -1, -1)    # x1 < x0: "no box" for the head of a multi-click prompt
REFINE_MARK = 4              # regions[4 i] of a refinement mark (dlimgedit.h: DLIMG_REFINE_MARK; csrc/prompt_plan.hpp: kRefineMark)
CLEAN_MARK = 6               # regions[4 i] of a clean-up mark (dlimgedit.h: DLIMG_CLEAN_MARK; csrc/prompt_plan.hpp: kCleanMark)
GRID_MARK = 7                # regions[4 i] of a grid mark (dlimgedit.h: DLIMG_GRID_MARK; csrc/grid_plan.hpp: kGridMark)
GRID_MAX_SIDE = 32
PRIOR_MARK = 8               # regions[4 i] of a prior mark (dlimgedit.h: DLIMG_PRIOR_MARK; csrc/prior_plan.hpp: kPriorMark)
PRIOR_MAX_STRENGTH = 100000  # strength_milli of a prior mark, at most; 0: the library's default (8000)
LASSO_MARK = 10              # regions[4 i] of a lasso mark (dlimgedit.h: DLIMG_LASSO_MARK; csrc/lasso_plan.hpp: kLassoMark)
LASSO_BOX, LASSO_CLICK, LASSO_MASK = 1, 2, 4     # the bits of a lasso mark's `what`; 0: all three
MATTE_MARK = 11              # regions[4 i] of a matte mark (dlimgedit.h: DLIMG_MATTE_MARK; csrc/matte_plan.hpp: kMatteMark)
MATTE_MAX_RADIUS = 32
MATTE_MAX_EPS = 65025        # eps of a matte mark, at most, in squared grey levels; 0: the library's default
MATTE_DEFAULT_EPS = 650
STROKE_MARK = 12             # regions[4 i] of a stroke mark (dlimgedit.h: DLIMG_STROKE_MARK; csrc/stroke_plan.hpp: kStrokeMark)
STROKE_DEFAULT_CLICKS = 3    # clicks of a stroke mark that says 0
CUTOUT_MARK = 13             # regions[4 i] of a cut-out mark (dlimgedit.h: DLIMG_CUTOUT_MARK; csrc/cutout_plan.hpp: kCutoutMark)
CUTOUT_MAX_RADIUS = 32
CUTOUT_DEFAULT_RADIUS = 16   # radius of a cut-out mark that says 0
EDGE_MARK = 14               # regions[4 i] of an edge mark (dlimgedit.h: DLIMG_EDGE_MARK; csrc/edge_plan.hpp: kEdgeMark)
EDGE_MAX_OFFSET = 64         # offset of an edge mark: -64 .. 64 pixels
EDGE_MAX_FEATHER = 32
EDGE_MAX_BORDER = 32


@dataclass
class ClickEntries:
    """The entry lists of one multi-click batch call, as table slot 14 and its device form read them: entry i has the handle
    index heads[i] (None: a continuation entry, one more click of the prompt in front of it), the click points[i] and the
    four ints regions[i] -- the box of a head (EMPTY_REGION: none), (label, 0, 0, 0) of a continuation entry.
    prompt_heads[j] is the entry that opened prompt j, token_rows[j] its token rows in the decoder (6 + clicks, 7 + clicks with
    a box), and launches the decoder launches of one GPU: [(token rows, [prompt indices])], prompts grouped by their token
    rows in order of first appearance and cut at the 112 rows a launch holds.
    A refinement mark is a continuation entry (REFINE_MARK, 0, 0, 0) whose point is not read.  stage_clicks[j]: the clicks each
    stage of prompt j takes (one stage without marks; token_rows[j] are the last stage's).  A prompt with marks is decoded
    behind the others, one launch per stage.
    A clean-up mark is a continuation entry (CLEAN_MARK, max_hole, max_island, 0), the last entry of its prompt, whose point is
    not read either: the prompt's mask is delivered with its small holes filled and its small islands dropped.  It changes
    neither token_rows nor stage_clicks nor launches.
    A grid prompt is two entries: a head with EMPTY_REGION and a continuation entry (GRID_MARK, side, iou_permille,
    stability_permille); neither point is read.  grid_sides[j]: the side of prompt j's grid, 0 for any other prompt.  It is
    decoded behind the others in launches of its own (side * side one-click prompts, 16 per launch), which `launches` does
    not list; token_rows[j] are those of one of its prompts.
    A prior mark is a continuation entry (PRIOR_MARK, strength_milli, 0, 0) directly behind its head, whose point is not read
    and whose out_masks pointer is READ: priors[j] is the (h, w) uint8 mask prompt j hands in as SAM's mask input of its first
    stage, None for a prompt without one.  A prompt with a prior is decoded behind the others like a prompt with marks, its
    first stage masked too; token_rows and stage_clicks are unchanged.
    A lasso mark is a continuation entry (LASSO_MARK, strength_milli, what, 0) directly behind its head, whose out_masks pointer is
    READ likewise: lassos[j] is the (h, w) uint8 selection of prompt j, None without one.  Its box and / or first click are
    derived on the GPU: token_rows and stage_clicks count the derived click (it belongs to the first stage) and the derived
    box.  Such a prompt is decoded behind the others like a prompt with marks.
    A matte mark is a continuation entry (MATTE_MARK, radius, eps, channels), the last entry of its prompt (behind the clean-up
    mark), whose out_masks pointer is READ as well: mattes[j] is the (h, w[, c]) uint8 image that guides the soft edge of prompt
    j's mask, None without one.  It changes neither token_rows nor stage_clicks; such a prompt is decoded on its own.
    A stroke mark is a continuation entry (STROKE_MARK, clicks, label, 0) behind the prompt's clicks, whose out_masks pointer is
    READ as a stroke map: strokes[j] are the (h, w) uint8 maps of prompt j's marks in their order, [] without one.  Each stands
    for `clicks` clicks (0: STROKE_DEFAULT_CLICKS) of its label, derived on the GPU: token_rows and stage_clicks count them (they
    belong to the last stage).  When the prompts of a call have strokes and no clicks, `points` is None and the first foreground
    click of every prompt is its head's.  Such a prompt is decoded behind the others like a prompt with marks.
    A cut-out mark is a continuation entry (CUTOUT_MARK, radius, 0, 0) directly behind the matte mark, the last entry of its
    prompt then, whose out_masks pointer is WRITTEN: cutouts[j] is (radius, the (h, w, 4) uint8 array that receives prompt j's
    foreground colours and coverage), None without one.  It changes nothing else.
    An edge mark is a continuation entry (EDGE_MARK, offset, feather, border) behind the clicks and the clean-up mark of its prompt
    and in front of its matte mark, whose point and pointer are not read: the prompt's mask is delivered grown, shrunk, feathered
    or bordered.  It changes neither token_rows nor stage_clicks nor launches."""
    heads: list
    points: list
    regions: list
    prompt_heads: list
    token_rows: list
    stage_clicks: list = field(default_factory=list)
    grid_sides: list = field(default_factory=list)
    priors: list = field(default_factory=list)
    lassos: list = field(default_factory=list)
    mattes: list = field(default_factory=list)
    strokes: list = field(default_factory=list)
    cutouts: list = field(default_factory=list)

    def _staged(self, j) -> bool:
        return (j < len(self.stage_clicks) and len(self.stage_clicks[j]) > 1) or (j < len(self.priors) and self.priors[j] is not None) \
            or (j < len(self.lassos) and self.lassos[j] is not None) or (j < len(self.mattes) and self.mattes[j] is not None) \
            or (j < len(self.strokes) and len(self.strokes[j]) > 0)

    def _grid(self, j) -> bool:
        return j < len(self.grid_sides) and self.grid_sides[j] > 0

    @property
    def launches(self) -> list:
        out = []
        plain = [j for j in range(len(self.token_rows)) if not self._staged(j) and not self._grid(j)]
        for t in dict.fromkeys(self.token_rows[j] for j in plain):
            group = [j for j in plain if self.token_rows[j] == t]
            cut = TOKEN_ROWS_MAX // t
            out += [(t, group[k:k + cut]) for k in range(0, len(group), cut)]
        for j in range(len(self.token_rows)):
            if self._staged(j):
                box_rows = self.token_rows[j] - self.stage_clicks[j][-1]
                out += [(box_rows + k, [j]) for k in self.stage_clicks[j]]
        return out


def pack_clicks(clicks, labels, region=None):
    """One prompt as the decoder sees it, in the order SAM's PromptEncoder packs it: the clicks in the order given with labels
    1 (foreground) / 0 (background), then the box's top-left and bottom-right (labels 2, 3); the padding point (0, 0) with label
    -1 only when there is no box.  -> ([(x, y)], [label]) in image pixels."""
    clicks, labels = _checked_clicks(clicks, labels)
    pts = [(c.x, c.y) for c in clicks]
    labs = list(labels)
    if region is not None:
        pts += [(region.top_left.x, region.top_left.y), (region.bottom_right.x, region.bottom_right.y)]
        labs += [2, 3]
    else:
        pts.append((0, 0))
        labs.append(-1)
    return pts, labs


def _checked_clicks(clicks, labels):
    clicks = list(clicks)
    labels = [1] * len(clicks) if labels is None else [int(v) for v in labels]
    if not clicks:
        raise Error("a prompt needs at least one click")
    if len(clicks) > MAX_CLICKS:
        raise Error(f"a prompt takes at most {MAX_CLICKS} clicks, not {len(clicks)}")
    if len(labels) != len(clicks):
        raise Error(f"{len(clicks)} clicks but {len(labels)} labels")
    if any(v not in (0, 1) for v in labels):
        raise Error("the label of a click is 1 (foreground) or 0 (background)")
    if labels[0] != 1:
        raise Error("the first click of a prompt is a foreground click: it travels in the head entry, which has no label")
    return clicks, labels


def _checked_marks(n_clicks: int, refine_after) -> list:
    """`refine_after` of one prompt -> the click counts behind which a refinement mark goes: None: none; "each": one behind
    every click but the last (SAM's interactive loop); else click counts k, strictly increasing, 1 <= k < the prompt's clicks."""
    if refine_after is None:
        return []
    if isinstance(refine_after, str):
        if refine_after != "each":
            raise Error('refine_after is a sequence of click counts or "each"')
        return list(range(1, n_clicks))
    ks = [int(k) for k in refine_after]
    if any(k < 1 or k >= n_clicks for k in ks):
        raise Error(f"refine_after: a mark goes behind the first k clicks, 1 <= k < {n_clicks} (every stage adds at least one click)")
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise Error("refine_after: the click counts are strictly increasing (no mark directly after another)")
    return ks


def _checked_clean(clean, n: int) -> list:
    """`clean` of a call of n prompts -> per prompt None or (max_hole, max_island): None: no prompt is cleaned; one pair of
    ints: every prompt; else one entry (None or a pair) per prompt.  Thresholds are pixels of the delivered mask, >= 0 and not
    both 0 (what the library refuses is refused here, before anything reaches it)."""
    if clean is None:
        return [None] * n
    def pair(c):
        c = tuple(c)
        if len(c) != 2 or not all(isinstance(v, (int, np.integer)) for v in c):
            raise Error("clean: a clean-up mark is a pair of ints (max_hole, max_island)")
        a, b = int(c[0]), int(c[1])
        if a < 0 or b < 0 or (a == 0 and b == 0):
            raise Error("clean: a clean-up mark has max_hole >= 0 and max_island >= 0, not both 0")
        if max(a, b) > 0x7fffffff:
            raise Error("clean: a clean-up mark's thresholds are C ints")
        return a, b

    clean = list(clean)
    if len(clean) == 2 and all(isinstance(v, (int, np.integer)) for v in clean):
        return [pair(clean)] * n
    if len(clean) != n:
        raise Error("clean: None, one (max_hole, max_island) pair for all prompts, or one entry (None or a pair) per prompt")
    return [None if c is None else pair(c) for c in clean]


def _checked_grid(grid, n: int) -> list:
    """`grid` of a call of n prompts -> per prompt None or (side, iou_permille, stability_permille): None: no grid prompt; else
    one entry (None, or a triple of ints, side 1 .. 32) per prompt."""
    if grid is None:
        return [None] * n
    grid = list(grid)
    if len(grid) != n:
        raise Error("grid: None, or one entry (None or (side, iou_permille, stability_permille)) per prompt")

    def triple(g):
        g = tuple(g)
        if len(g) != 3 or not all(isinstance(v, (int, np.integer)) for v in g):
            raise Error("grid: a grid mark is three ints (side, iou_permille, stability_permille)")
        if not 1 <= int(g[0]) <= GRID_MAX_SIDE:
            raise Error(f"grid: the side of a grid mark is 1..{GRID_MAX_SIDE}")
        if any(abs(int(v)) > 0x7fffffff for v in g):
            raise Error("grid: a grid mark's thresholds are C ints")
        return int(g[0]), int(g[1]), int(g[2])
    return [None if g is None else triple(g) for g in grid]


def _checked_prior(prior, prior_strength, n: int) -> list:
    """`prior` / `prior_strength` of a call of n prompts -> per prompt None or ((h, w) uint8 array, strength_milli): prior is
    None or one entry (None or an array) per prompt; prior_strength one int for all or one per prompt, 0 .. 100000 (0: the
    library's default)."""
    if prior is None:
        return [None] * n
    prior = list(prior)
    if len(prior) != n:
        raise Error("prior: None, or one entry (None or an (h, w) uint8 array) per prompt")
    strengths = [prior_strength] * n if isinstance(prior_strength, (int, np.integer)) else list(prior_strength)
    if len(strengths) != n or not all(isinstance(v, (int, np.integer)) for v in strengths):
        raise Error("prior_strength: one int for all prompts or one per prompt")
    out = []
    for m, v in zip(prior, strengths):
        if m is None:
            out.append(None)
            continue
        if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.ndim != 2 or not m.flags.c_contiguous:
            raise Error("prior: a prior is a C-contiguous (h, w) uint8 array of the image's extent")
        if not 0 <= int(v) <= PRIOR_MAX_STRENGTH:
            raise Error(f"prior_strength: 0 (the default) .. {PRIOR_MAX_STRENGTH}")
        out.append((m, int(v)))
    return out


def _checked_lasso(lasso, lasso_what, lasso_strength, n: int) -> list:
    """`lasso` / `lasso_what` / `lasso_strength` of a call of n prompts -> per prompt None or ((h, w) uint8 array, what,
    strength_milli): lasso is None or one entry (None or an array) per prompt; lasso_what and lasso_strength one int for all or
    one per prompt.  what: a bit set of LASSO_BOX, LASSO_CLICK, LASSO_MASK, 0 (all) .. 7 other than 4; strength 0 .. 100000, 0
    without LASSO_MASK."""
    if lasso is None:
        return [None] * n
    lasso = list(lasso)
    if len(lasso) != n:
        raise Error("lasso: None, or one entry (None or an (h, w) uint8 array) per prompt")
    def per_prompt(v, name):
        vs = [v] * n if isinstance(v, (int, np.integer)) else list(v)
        if len(vs) != n or not all(isinstance(x, (int, np.integer)) for x in vs):
            raise Error(f"{name}: one int for all prompts or one per prompt")
        return [int(x) for x in vs]
    whats, strengths = per_prompt(lasso_what, "lasso_what"), per_prompt(lasso_strength, "lasso_strength")
    out = []
    for m, what, v in zip(lasso, whats, strengths):
        if m is None:
            out.append(None)
            continue
        if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.ndim != 2 or not m.flags.c_contiguous:
            raise Error("lasso: a selection is a C-contiguous (h, w) uint8 array of the image's extent")
        if not 0 <= what <= 7 or what == LASSO_MASK:
            raise Error("lasso_what: a bit set of LASSO_BOX, LASSO_CLICK and LASSO_MASK, 0 (all) .. 7; 4 alone derives nothing")
        if not 0 <= v <= PRIOR_MAX_STRENGTH or (v and what and not what & LASSO_MASK):
            raise Error(f"lasso_strength: 0 (the default) .. {PRIOR_MAX_STRENGTH}, and 0 without LASSO_MASK")
        out.append((m, what, v))
    return out


def _checked_matte(matte, n: int) -> list:
    """`matte` of a call of n prompts -> per prompt None or (image, channels, radius, eps): matte is None or one entry per prompt,
    None or (image, radius, eps) with image an (h, w), (h, w, 3) or (h, w, 4) C-contiguous uint8 array, radius 1 .. 32 and eps
    0 (the library's default) .. 65025."""
    if matte is None:
        return [None] * n
    matte = list(matte)
    if len(matte) != n:
        raise Error("matte: None, or one entry (None or (image, radius, eps)) per prompt")
    out = []
    for m in matte:
        if m is None:
            out.append(None)
            continue
        if not isinstance(m, (tuple, list)) or len(m) != 3:
            raise Error("matte: a matte is (image, radius, eps)")
        g, radius, eps = m
        if not isinstance(g, np.ndarray) or g.dtype != np.uint8 or not g.flags.c_contiguous or \
                not (g.ndim == 2 or (g.ndim == 3 and g.shape[2] in (1, 3, 4))):
            raise Error("matte: the guide is a C-contiguous (h, w), (h, w, 3) or (h, w, 4) uint8 array of the image's extent")
        if not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= MATTE_MAX_RADIUS:
            raise Error(f"matte: radius is 1 .. {MATTE_MAX_RADIUS}")
        if not isinstance(eps, (int, np.integer)) or not 0 <= int(eps) <= MATTE_MAX_EPS:
            raise Error(f"matte: eps is 0 (the default) .. {MATTE_MAX_EPS}")
        out.append((g, 1 if g.ndim == 2 else g.shape[2], int(radius), int(eps)))
    return out


def _checked_cutout(cutout, matte: list, n: int) -> list:
    """`cutout` of a call of n prompts whose checked mattes are `matte` -> per prompt None or (radius, out): cutout is None or
    one entry per prompt, None, a radius 0 (the library's default, 16) .. 32, or (radius, out) with out the C-contiguous
    (h, w, 4) uint8 array that receives the RGBA -- a new one without it.  The prompt has a matte whose image has 3 or 4
    channels; out may be that image itself when it has 4."""
    if cutout is None:
        return [None] * n
    cutout = list(cutout)
    if len(cutout) != n:
        raise Error("cutout: None, or one entry (None, a radius or (radius, out)) per prompt")
    out = []
    for j, q in enumerate(cutout):
        if q is None:
            out.append(None)
            continue
        radius, dst = q if isinstance(q, (tuple, list)) and len(q) == 2 else (q, None)
        if not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= CUTOUT_MAX_RADIUS:
            raise Error(f"cutout: a cut-out is a radius 0 (the default, {CUTOUT_DEFAULT_RADIUS}) .. {CUTOUT_MAX_RADIUS}, or (radius, out)")
        if matte[j] is None or matte[j][1] not in (3, 4):
            raise Error("cutout: a cut-out takes its colours from the prompt's matte image, which has 3 or 4 channels")
        shape = matte[j][0].shape[:2] + (4,)
        if dst is None:
            dst = np.empty(shape, np.uint8)
        if not isinstance(dst, np.ndarray) or dst.dtype != np.uint8 or not dst.flags.c_contiguous or dst.shape != shape:
            raise Error("cutout: out is a C-contiguous (h, w, 4) uint8 array of the image's extent")
        out.append((int(radius), dst))
    return out


def _checked_edge(edge, n: int) -> list:
    """`edge` of a call of n prompts -> per prompt None or (offset, feather, border): edge is None or one entry per prompt, None,
    an int offset or (offset, feather, border) with offset -64 .. 64, feather 0 .. 32, border 0 .. 32, not all three 0."""
    if edge is None:
        return [None] * n
    if isinstance(edge, (int, np.integer)):
        raise Error("edge: None, or one entry (None, an offset or (offset, feather, border)) per prompt")
    edge = list(edge)
    if len(edge) != n:
        raise Error("edge: None, or one entry (None, an offset or (offset, feather, border)) per prompt")
    out = []
    for q in edge:
        if q is None:
            out.append(None)
            continue
        q = (q, 0, 0) if isinstance(q, (int, np.integer)) else q
        if not isinstance(q, (tuple, list)) or len(q) != 3 or not all(isinstance(v, (int, np.integer)) for v in q):
            raise Error("edge: an edge is an int offset or (offset, feather, border)")
        offset, feather, border = (int(v) for v in q)
        if not -EDGE_MAX_OFFSET <= offset <= EDGE_MAX_OFFSET or not 0 <= feather <= EDGE_MAX_FEATHER or not 0 <= border <= EDGE_MAX_BORDER:
            raise Error(f"edge: offset is -{EDGE_MAX_OFFSET} .. {EDGE_MAX_OFFSET}, feather 0 .. {EDGE_MAX_FEATHER}, border 0 .. {EDGE_MAX_BORDER}")
        if (offset, feather, border) == (0, 0, 0):
            raise Error("edge: offset, feather and border all 0 is the identity: pass None")
        out.append((offset, feather, border))
    return out


def _with_cutouts(outs: list, cutouts: list) -> list:
    """The results of a batch call: the mask of a prompt, (coverage, rgba) of one with a cut-out."""
    return [o if q is None else (o, q[1]) for o, q in zip(outs, cutouts)]


def _checked_strokes(strokes, n: int) -> list:
    """`strokes` of a call of n prompts -> per prompt a list of ((h, w) uint8 array, label, clicks), empty without strokes:
    strokes is None or one entry per prompt, None or a sequence of (map, label, clicks) with label 1 (foreground) or 0
    (background) and clicks 0 (the library's default, 3) .. 8."""
    if strokes is None:
        return [[] for _ in range(n)]
    strokes = list(strokes)
    if len(strokes) != n:
        raise Error("strokes: None, or one entry (None or a list of (map, label, clicks)) per prompt")
    out = []
    for marks in strokes:
        if marks is None:
            out.append([])
            continue
        if not isinstance(marks, (list, tuple)) or any(not isinstance(q, (list, tuple)) or len(q) != 3 for q in marks):
            raise Error("strokes: the strokes of a prompt are a list of (map, label, clicks)")
        checked = []
        for m, label, clicks in marks:
            if not isinstance(m, np.ndarray) or m.dtype != np.uint8 or m.ndim != 2 or not m.flags.c_contiguous:
                raise Error("strokes: a stroke map is a C-contiguous (h, w) uint8 array of the image's extent")
            if not isinstance(label, (int, np.integer)) or int(label) not in (0, 1):
                raise Error("strokes: the label of a stroke is 1 (foreground) or 0 (background)")
            if not isinstance(clicks, (int, np.integer)) or not 0 <= int(clicks) <= MAX_CLICKS:
                raise Error(f"strokes: clicks is 0 (the default, {STROKE_DEFAULT_CLICKS}) .. {MAX_CLICKS}")
            checked.append((m, int(label), int(clicks)))
        out.append(checked)
    return out


def _entry_pointers(segs, heads, regs, outs_by_head: dict, priors: list, lassos: Optional[list] = None,
                    mattes: Optional[list] = None, strokes: Optional[list] = None, cutouts: Optional[list] = None) -> list:
    """out_masks of a call: the result of a head entry, the prior of a prior mark (priors by index into segs), the selection of
    a lasso mark (lassos likewise), the guide of a matte mark (mattes likewise), the map of a stroke mark (strokes likewise, the
    marks of a prompt in their order), the destination of a cut-out mark (cutouts likewise), None otherwise."""
    ptrs, head, mark = [], None, 0
    for e, h in enumerate(heads):
        if h is not None:
            head, mark = h, 0
            ptrs.append(outs_by_head[e].ctypes.data)
        elif regs[e][0] == STROKE_MARK and head is not None and strokes is not None and mark < len(strokes[head]):
            m, ext = strokes[head][mark][0], segs[head].extent()
            mark += 1
            if m.shape != (ext.height, ext.width):
                raise Error(f"strokes: a stroke map of prompt {head} is {m.shape[1]} x {m.shape[0]}, its image {ext.width} x {ext.height}")
            ptrs.append(m.ctypes.data)
        elif regs[e][0] == PRIOR_MARK and head is not None and priors[head] is not None:
            m, ext = priors[head][0], segs[head].extent()
            if m.shape != (ext.height, ext.width):
                raise Error(f"prior: the prior of prompt {head} is {m.shape[1]} x {m.shape[0]}, its image {ext.width} x {ext.height}")
            ptrs.append(m.ctypes.data)
        elif regs[e][0] == LASSO_MARK and head is not None and lassos is not None and lassos[head] is not None:
            m, ext = lassos[head][0], segs[head].extent()
            if m.shape != (ext.height, ext.width):
                raise Error(f"lasso: the selection of prompt {head} is {m.shape[1]} x {m.shape[0]}, its image {ext.width} x {ext.height}")
            ptrs.append(m.ctypes.data)
        elif regs[e][0] == MATTE_MARK and head is not None and mattes is not None and mattes[head] is not None:
            g, ext = mattes[head][0], segs[head].extent()
            if g.shape[:2] != (ext.height, ext.width):
                raise Error(f"matte: the guide of prompt {head} is {g.shape[1]} x {g.shape[0]}, its image {ext.width} x {ext.height}")
            ptrs.append(g.ctypes.data)
        elif regs[e][0] == CUTOUT_MARK and head is not None and cutouts is not None and cutouts[head] is not None:
            ptrs.append(cutouts[head][1].ctypes.data)
        else:
            ptrs.append(None)
    return ptrs


def _marked_entries(n: int, points, regions, clean: list, grid: Optional[list] = None, prior: Optional[list] = None,
                    lasso: Optional[list] = None, matte: Optional[list] = None, cutout: Optional[list] = None,
                    edge: Optional[list] = None):
    """The `points` / `regions` form of a batch call with clean-up, grid or prior marks as entry lists: entry i of the caller's,
    then its marks (the prior mark first: it stands directly behind its head).  -> (index into segs or None per entry, [(x, y)]
    or None, [(4 ints)]).  A point prompt gets the empty region (no box); a grid prompt is its head with the empty region and
    its mark (its point and region, if any were given, are not used)."""
    heads, pts, regs = [], ([] if points is not None else None), []
    for i in range(n):
        heads.append(i)
        if pts is not None:
            pts.append((points[i].x, points[i].y) if points[i] is not None else (0, 0))
        if grid is not None and grid[i] is not None:
            if clean[i] is not None:
                raise Error("a grid prompt takes no clean-up mark")
            if prior is not None and prior[i] is not None:
                raise Error("a grid prompt takes no prior")
            if lasso is not None and lasso[i] is not None:
                raise Error("a grid prompt takes no lasso")
            if matte is not None and matte[i] is not None:
                raise Error("a grid prompt takes no matte: a label map is not a coverage")
            if edge is not None and edge[i] is not None:
                raise Error("a grid prompt takes no edge mark: a label map has no edge to move")
            regs.append(EMPTY_REGION)
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((GRID_MARK,) + tuple(grid[i]))
            continue
        q = None if regions is None else regions[i]
        regs.append(EMPTY_REGION if q is None else (q.top_left.x, q.top_left.y, q.bottom_right.x, q.bottom_right.y))
        if prior is not None and prior[i] is not None:
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((PRIOR_MARK, prior[i][1], 0, 0))
        if lasso is not None and lasso[i] is not None:
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((LASSO_MARK, lasso[i][2], lasso[i][1], 0))
        if clean[i] is not None:
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((CLEAN_MARK, clean[i][0], clean[i][1], 0))
        if edge is not None and edge[i] is not None:          # behind the clean-up mark, in front of the matte mark
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((EDGE_MARK,) + tuple(edge[i]))
        if matte is not None and matte[i] is not None:        # behind everything else of its prompt
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((MATTE_MARK, matte[i][2], matte[i][3], matte[i][1]))
        if cutout is not None and cutout[i] is not None:      # directly behind the matte mark
            heads.append(None)
            if pts is not None:
                pts.append((0, 0))
            regs.append((CUTOUT_MARK, cutout[i][0], 0, 0))
    return heads, pts, regs


def _marked_arrays(segs, heads, pts, regs):
    n = len(heads)
    handles = (C.c_void_p * n)(*[None if h is None else segs[h]._handle for h in heads])
    p = None if pts is None else (C.c_int * (2 * n))(*[v for q in pts for v in q])
    r = (C.c_int * (4 * n))(*[v for q in regs for v in q])
    return n, handles, p, r


def click_entries(clicks, labels=None, regions=None, refine_after=None, clean=None, grid=None, prior=None,
                  prior_strength=0, lasso=None, lasso_what=0, lasso_strength=0, matte=None, strokes=None,
                  cutout=None, edge=None) -> ClickEntries:
    """Entry lists for prompts of several clicks: clicks[j] the Points of prompt j (1 .. 8, the first one foreground),
    labels[j] their labels (None: all foreground), regions[j] its box or None.  refine_after: None, "each" (for every
    prompt), or per prompt None / "each" / click counts k -- "a refinement mark after the first k clicks": the prompt is then
    decoded in stages, each taking the low-res logits of the one before it as SAM's mask input.  clean: None, one
    (max_hole, max_island) pair for every prompt, or per prompt None / a pair -- a clean-up mark behind the prompt's last click.
    grid: None, or per prompt None / (side, iou_permille, stability_permille) -- prompt j is a grid prompt ("segment
    everything"): clicks[j] is None or empty, and it takes no labels, region, refinement or clean-up marks.
    prior: None, or per prompt None / an (h, w) uint8 mask of the prompt's image -- a prior mark directly behind the head, with
    prior_strength (one int for all or one per prompt; 0: the library's default) as its strength_milli.  Entry lists without
    priors are what they were.
    lasso: None, or per prompt None / an (h, w) uint8 selection of the prompt's image -- a lasso mark directly behind the head,
    with lasso_what (bits LASSO_BOX, LASSO_CLICK, LASSO_MASK; 0: all) and lasso_strength (0 without LASSO_MASK), one int for
    all or one per prompt.  clicks[j] are then the clicks BEHIND the derived one (the entry lists always carry `points`, so
    there is at least one; a lasso alone is Segmentation.snap_selection), and refine_after counts the clicks given.  Entry
    lists without lasso marks are what they were.
    matte: None, or per prompt None / (image, radius, eps) -- a matte mark, the last entry of its prompt: the mask is delivered
    as coverage 0 .. 255, its edge guided by the image (see compute_mask_clicks).  Entry lists without matte marks are what
    they were.
    strokes: None, or per prompt None / a list of (map, label, clicks) -- stroke marks behind the prompt's clicks, in front of
    its clean-up mark: map an (h, w) uint8 scribble over the prompt's image (a pixel belongs to it from 128 on), label 1
    (foreground) or 0 (background), clicks 1 .. 8 clicks to sample from it on the GPU, 0: the default 3.  The derived clicks count
    towards the 8; refine_after counts the clicks given.  A prompt with strokes may have NO clicks (clicks[j] None): then no prompt
    of the call has any, every one has a foreground stroke, whose first click is its head's, and the entry lists carry no
    `points`.  Entry lists without strokes are what they were.
    cutout: None, or per prompt None / a radius / (radius, out) -- a cut-out mark directly behind the prompt's matte mark (which
    it needs, with an image of 3 or 4 channels): the image's foreground colours under the matte's coverage, as RGBA (see
    compute_mask_clicks).  Entry lists without cut-outs are what they were.
    edge: None, or per prompt None / an int offset / (offset, feather, border) -- an edge mark behind the prompt's clean-up mark
    and in front of its matte mark: the mask grown, shrunk, feathered or bordered (see compute_mask_clicks).  Entry lists without
    edge marks are what they were.
    Pure host code."""
    n = len(clicks)
    strokes = _checked_strokes(strokes, n)
    any_stroke = any(strokes)
    clickless = [bool(strokes[j]) and not clicks[j] for j in range(n)]
    clean = _checked_clean(clean, n)
    grid = _checked_grid(grid, n)
    prior = _checked_prior(prior, prior_strength, n)
    any_prior = any(p is not None for p in prior)
    lasso = _checked_lasso(lasso, lasso_what, lasso_strength, n)
    any_lasso = any(q is not None for q in lasso)
    matte = _checked_matte(matte, n)
    any_matte = any(q is not None for q in matte)
    cutout = _checked_cutout(cutout, matte, n)
    any_cutout = any(q is not None for q in cutout)
    edge = _checked_edge(edge, n)
    labels = [None] * n if labels is None else list(labels)
    regions = [None] * n if regions is None else list(regions)
    refine_after = [refine_after] * n if refine_after is None or isinstance(refine_after, str) else list(refine_after)
    if len(labels) != n or len(regions) != n or len(refine_after) != n:
        raise Error("one list of labels, one region (or None) and one refine_after (or None) per prompt")
    out = ClickEntries([], [], [], [], [])
    for j in range(n):
        out.grid_sides.append(0 if grid[j] is None else grid[j][0])
        if any_prior:
            out.priors.append(None if prior[j] is None else prior[j][0])
        if any_lasso:
            out.lassos.append(None if lasso[j] is None else lasso[j][0])
        if any_matte:
            out.mattes.append(None if matte[j] is None else matte[j][0])
        if any_cutout:
            out.cutouts.append(cutout[j])
        if grid[j] is not None and lasso[j] is not None:
            raise Error("a grid prompt takes no lasso")
        if grid[j] is not None and matte[j] is not None:
            raise Error("a grid prompt takes no matte: a label map is not a coverage")
        if grid[j] is not None and strokes[j]:
            raise Error("a grid prompt takes no strokes")
        if grid[j] is not None and edge[j] is not None:
            raise Error("a grid prompt takes no edge mark: a label map has no edge to move")
        if any_stroke:
            out.strokes.append([q[0] for q in strokes[j]])
        if grid[j] is not None:
            if clicks[j] or labels[j] is not None or regions[j] is not None or refine_after[j] is not None or clean[j] is not None \
                    or prior[j] is not None:
                raise Error("a grid prompt is its grid mark alone: no clicks, labels, region, refinement or clean-up marks, no prior")
            out.prompt_heads.append(len(out.heads))
            out.token_rows.append(7)
            out.stage_clicks.append([1])
            out.heads += [j, None]
            out.points += [(0, 0), (0, 0)]
            out.regions += [EMPTY_REGION, (GRID_MARK,) + grid[j]]
            continue
        if clickless[j]:
            if labels[j] or refine_after[j] is not None:
                raise Error("strokes: labels and refine_after go with the clicks given, and this prompt has none")
            if not any(label == 1 for _, label, _ in strokes[j]):
                raise Error("strokes: background strokes alone are no prompt: without clicks a prompt needs a foreground stroke")
            cs, ls = [], []
        else:
            cs, ls = _checked_clicks(clicks[j], labels[j])
        marks = _checked_marks(len(cs), refine_after[j])
        r = regions[j]
        sampled = sum(q[2] or STROKE_DEFAULT_CLICKS for q in strokes[j])
        out.prompt_heads.append(len(out.heads))
        what = 0 if lasso[j] is None else (lasso[j][1] or 7)
        if what and prior[j] is not None:
            raise Error("a prompt takes a prior or a lasso, not both")
        if what & LASSO_BOX and r is not None:
            raise Error("lasso: with LASSO_BOX the prompt's box is the selection's: no region")
        derived = 1 if what & LASSO_CLICK else 0
        if derived + len(cs) + sampled > MAX_CLICKS:
            raise Error(f"a prompt takes at most {MAX_CLICKS} clicks, the clicks its strokes stand for counted: not {derived + len(cs) + sampled}")
        out.token_rows.append(5 + derived + len(cs) + sampled + (2 if r is not None or what & LASSO_BOX else 1))
        out.stage_clicks.append([k + derived for k in marks] + [derived + len(cs) + sampled])
        if clickless[j]:                     # the head alone: its click will be the first foreground click of its strokes
            out.heads.append(j)
            out.points.append((0, 0))
            out.regions.append(EMPTY_REGION if r is None else (r.top_left.x, r.top_left.y, r.bottom_right.x, r.bottom_right.y))
            if prior[j] is not None:
                out.heads.append(None)
                out.points.append((0, 0))
                out.regions.append((PRIOR_MARK, prior[j][1], 0, 0))
            if lasso[j] is not None:
                out.heads.append(None)
                out.points.append((0, 0))
                out.regions.append((LASSO_MARK, lasso[j][2], lasso[j][1], 0))
        for k, (c, lab) in enumerate(zip(cs, ls)):
            if k in marks:               # a mark behind the first k clicks: in front of click k (0-based)
                out.heads.append(None)
                out.points.append((0, 0))
                out.regions.append((REFINE_MARK, 0, 0, 0))
            out.heads.append(j if k == 0 else None)
            out.points.append((c.x, c.y))
            if k:
                out.regions.append((lab, 0, 0, 0))
            else:
                out.regions.append(EMPTY_REGION if r is None else (r.top_left.x, r.top_left.y, r.bottom_right.x, r.bottom_right.y))
                if prior[j] is not None:     # the prior mark stands directly behind its head
                    out.heads.append(None)
                    out.points.append((0, 0))
                    out.regions.append((PRIOR_MARK, prior[j][1], 0, 0))
                if lasso[j] is not None:     # so does the lasso mark
                    out.heads.append(None)
                    out.points.append((0, 0))
                    out.regions.append((LASSO_MARK, lasso[j][2], lasso[j][1], 0))
        for _, label, n_clicks in strokes[j]:    # behind the clicks given, in front of the marks that stay last
            out.heads.append(None)
            out.points.append((0, 0))
            out.regions.append((STROKE_MARK, n_clicks, label, 0))
        if clean[j] is not None:
            out.heads.append(None)
            out.points.append((0, 0))
            out.regions.append((CLEAN_MARK, clean[j][0], clean[j][1], 0))
        if edge[j] is not None:              # behind the clean-up mark, in front of the matte mark
            out.heads.append(None)
            out.points.append((0, 0))
            out.regions.append((EDGE_MARK,) + edge[j])
        if matte[j] is not None:             # behind everything else of its prompt
            out.heads.append(None)
            out.points.append((0, 0))
            out.regions.append((MATTE_MARK, matte[j][2], matte[j][3], matte[j][1]))
        if cutout[j] is not None:            # directly behind the matte mark
            out.heads.append(None)
            out.points.append((0, 0))
            out.regions.append((CUTOUT_MARK, cutout[j][0], 0, 0))
    if any(clickless):
        # a call without `points`: every prompt takes its head's click from a foreground stroke (dlimgedit.h, DLIMG_STROKE_MARK)
        if not all(clickless):
            raise Error("strokes: a prompt with strokes and no clicks travels in a call without `points`, so no prompt of the call has "
                        "clicks and every one has a foreground stroke")
        out.points = None
    return out


def _entry_calls(entries: ClickEntries) -> list:
    """The calls that carry `entries`: [[entry indices], regions given].  One call with both arrays as soon as any prompt has a
    second click.  Without any, the entries are today's point and box + point entries, in which an empty region has no
    special meaning: the prompts without a box travel in a call without `regions`, those with one in a call with both."""
    n = len(entries.heads)
    if any(h is None for h in entries.heads):
        return [(list(range(n)), True)]
    plain = [i for i in range(n) if entries.regions[i] == EMPTY_REGION]
    boxed = [i for i in range(n) if entries.regions[i] != EMPTY_REGION]
    return [(sel, given) for sel, given in ((plain, False), (boxed, True)) if sel]


def _entry_arrays(segs, entries: ClickEntries, sel, regions_given: bool):
    n = len(sel)
    handles = (C.c_void_p * n)(*[None if entries.heads[i] is None else segs[entries.heads[i]]._handle for i in sel])
    p = None if entries.points is None else (C.c_int * (2 * n))(*[v for i in sel for v in entries.points[i]])
    r = (C.c_int * (4 * n))(*[v for i in sel for v in entries.regions[i]]) if regions_given else None
    return n, handles, p, r


class Segmentation:
    """dlimg::Segmentation: cached image embedding + mask queries."""

    def __init__(self, handle: C.c_void_p, env: Environment):
        self._handle, self._env = handle, env   # keeps the environment alive

    @staticmethod
    def process(img: ImageView, env: Environment) -> "Segmentation":
        seg = Segmentation(C.c_void_p(), env)
        v = img._c()
        # the handle is assigned before encoding: on failure the wrapper still owns and frees it
        _check(api().process_image_for_segmentation(C.byref(seg._handle), C.byref(v), env.handle()))
        return seg

    @staticmethod
    def process_batch(imgs: Sequence[ImageView], env: Environment) -> list:
        n = len(imgs)
        handles = (C.c_void_p * n)()
        views = (_ImageView * n)(*[i._c() for i in imgs])
        segs = []
        try:
            _check(api().process_images_for_segmentation(handles, views, n, env.handle()))
        finally:
            segs = [Segmentation(C.c_void_p(h), env) for h in handles if h]
        return segs

    def extent(self) -> Extent:
        out = (C.c_int * 2)()
        api().get_segmentation_extent(self._handle, out)
        return Extent(out[0], out[1])

    def _query(self, point, region, n_masks, out=None):
        e = self.extent()
        masks = [_mask_image(e) for _ in range(n_masks)] if out is None else list(out)
        assert len(masks) == n_masks and all(m.shape == (e.height, e.width) and m.dtype == np.uint8 and
                                              m.flags.c_contiguous for m in masks)
        ptrs = (C.c_void_p * 3)(*([m.ctypes.data for m in masks] + [None] * (3 - n_masks)))
        acc = (C.c_float * 3)(0.0, 0.0, 0.0)
        p = (C.c_int * 2)(point.x, point.y) if point is not None else None
        r = (C.c_int * 4)(region.top_left.x, region.top_left.y, region.bottom_right.x, region.bottom_right.y) \
            if region is not None else None
        _check(api().get_segmentation_mask(self._handle, p, r, ptrs, acc))
        return masks, list(acc)

    def compute_mask(self, prompt, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Point -> best mask; Region -> mask of the largest object in the box.  `out`: the caller's own (h, w) uint8 buffer
        (the wrapper's compute_mask(point, uint8_t*) form) instead of a new Image of the library."""
        outs = None if out is None else [out]
        if isinstance(prompt, Point):
            return self._query(prompt, None, 1, outs)[0][0]
        if isinstance(prompt, Region):
            return self._query(None, prompt, 1, outs)[0][0]
        raise TypeError("prompt must be a Point or a Region")

    def compute_masks(self, point: Point) -> list:
        masks, acc = self._query(point, None, 3)
        return [Mask(m, a) for m, a in zip(masks, acc)]

    def segment_everything(self, side: int = 32, iou_permille: int = 0, stability_permille: int = 0,
                           out: Optional[np.ndarray] = None) -> np.ndarray:
        """Segment everything: the label map of a side x side point grid (1 .. 32) -- (h, w) uint8, 0 where no segment lies, k in
        1 .. 255 for the k-th kept segment, the smallest segment on top.  Candidates (outputs 1 .. 3 of every grid prompt) are kept
        whose predicted IoU is at least iou_permille / 1000 and whose stability at least stability_permille / 1000 (0: SAM's
        defaults, 880 and 950), and that box NMS at 0.7 leaves (dlimgedit.h, DLIMG_GRID_MARK)."""
        return Segmentation.compute_mask_batch([self], grid=[(side, iou_permille, stability_permille)],
                                               out=None if out is None else [out])[0]

    def compute_mask_clicks(self, clicks: Sequence[Point], labels: Optional[Sequence[int]] = None,
                            region: Optional[Region] = None, out: Optional[np.ndarray] = None, refine_after=None,
                            clean=None, prior: Optional[np.ndarray] = None, prior_strength: int = 0,
                            lasso: Optional[np.ndarray] = None, lasso_what: int = 0, lasso_strength: int = 0,
                            matte=None, strokes=None, cutout=None, edge=None):
        """Click-to-refine: one mask from 1 .. 8 clicks, labels[k] 1 (foreground, the first one always) or 0 (background), and
        an optional box.  With two clicks or more, or a box, the mask is the decoder's output 0.
        refine_after: click counts k, or "each" -- the clicks are replayed in stages as SAM's interactive predictor would take
        them: the first k clicks give a mask whose low-res logits are the mask input of the next stage (on the GPU), and so on;
        the mask of the last stage is returned.  Needs a model with the mask branch (pe.mask.*).
        clean: (max_hole, max_island) -- the mask is delivered with background components below max_hole pixels filled and then
        foreground components below max_island pixels dropped (8-connectivity; the largest island stays when all are below).
        prior: an (h, w) uint8 mask the caller already holds (a selection, the mask of the last query; 0 .. 255 read as
        coverage) as SAM's mask input of the first stage; it may be `out` itself, a mask refined in place.  prior_strength: the
        logit a fully covered pixel stands for, in thousandths, 1 .. 100000; 0: the library's default, 8000.  Needs a model
        with the mask branch.
        lasso: an (h, w) uint8 selection from which the prompt's box (LASSO_BOX), its first click (LASSO_CLICK: the most interior
        point, in front of `clicks`) and its first mask input (LASSO_MASK, at lasso_strength) are derived on the GPU;
        lasso_what 0: all three.  See snap_selection.
        matte: (image, radius, eps) -- the mask is delivered as COVERAGE 0 .. 255 instead of 0 / 255: the mask this prompt would
        deliver without it (cleaned, with `clean`) put through He et al.'s guided filter on the GPU, in integers, so that its
        edge follows the picture (dlimgedit.h, DLIMG_MATTE_MARK).  image: the image this segmentation was made from, an
        (h, w), (h, w, 3) or (h, w, 4) uint8 array (RGBA and BGRA give the same matte); radius 1 .. 32 pixels; eps 1 .. 65025
        squared grey levels, 0: the library's default, 650.
        strokes: a list of (map, label, clicks) -- scribbles over this image, (h, w) uint8 maps whose pixels belong to the stroke
        from 128 on, each standing for `clicks` clicks (1 .. 8, 0: the default 3) of its label (1 foreground, 0 background) that
        are sampled from it on the GPU, behind `clicks` (dlimgedit.h, DLIMG_STROKE_MARK).  With strokes, `clicks` may be None:
        the first foreground click sampled is then the prompt's first.  See scribble.
        cutout (with matte, whose image has 3 or 4 channels): a radius 1 .. 32 pixels (0: the default, 16), or (radius, out) --
        the call returns (coverage, rgba): rgba an (h, w, 4) uint8 array (`out`, a C-contiguous one of the caller's, which may be
        the matte's 4-channel image itself: decontaminated in place) whose first three bytes are the FOREGROUND colour of the
        pixel in the image's channel order -- one pass of Blur-Fusion over that radius on the GPU, in integers, which takes the
        old background out of the soft edge -- and whose fourth byte is the coverage (dlimgedit.h, DLIMG_CUTOUT_MARK).
        edge: an int offset, or (offset, feather, border) -- the mask (cleaned, with `clean`) is grown (offset > 0) or shrunk
        (offset < 0) by that many pixels, -64 .. 64, with a disc; feathered by a linear ramp 2 * feather pixels wide, 0 .. 32; or
        turned into a band of `border` pixels, 0 .. 32, on each side of the moved edge -- by an exact Euclidean distance on the
        GPU, in integers (dlimgedit.h, DLIMG_EDGE_MARK).  A mask that touches the image's border is not shrunk from it.  With
        `matte`, the matte filters what the edge mark delivered: shrink in front of it against a halo."""
        return Segmentation.compute_mask_batch([self], clicks=[clicks], labels=[labels], regions=[region],
                                               edge=None if edge is None else [edge],
                                               cutout=None if cutout is None else [cutout],
                                               strokes=None if strokes is None else [list(strokes)],
                                               out=None if out is None else [out],
                                               refine_after=None if refine_after is None else [refine_after],
                                               clean=None if clean is None else [tuple(clean)],
                                               prior=None if prior is None else [prior], prior_strength=prior_strength,
                                               lasso=None if lasso is None else [lasso], lasso_what=lasso_what,
                                               lasso_strength=lasso_strength, matte=None if matte is None else [tuple(matte)])[0]

    def snap_selection(self, mask: np.ndarray, what: int = 0, strength: int = 0, clicks: Optional[Sequence[Point]] = None,
                       labels: Optional[Sequence[int]] = None, refine_after=None, clean=None,
                       out: Optional[np.ndarray] = None, matte=None, cutout=None, edge=None):
        """Snap a selection to the object: mask, an (h, w) uint8 selection of this image (a dragged lasso, a painted blob; 0 ..
        255 read as coverage), is the prompt -- its box (LASSO_BOX), its most interior point as a foreground click
        (LASSO_CLICK) and the selection itself as SAM's mask input (LASSO_MASK, at `strength` thousandths, 0: the default
        8000; needs a model with the mask branch), whichever bits `what` holds, 0: all three.  Box and click are derived on
        the GPU from the 256 x 256 low-res grid (dlimgedit.h, DLIMG_LASSO_MARK).  clicks / labels: further clicks behind the
        derived one (the first of them foreground); refine_after counts these; clean as for compute_mask_clicks.  `out` may be
        `mask` itself: a selection snapped in place.  An empty selection (no low-res cell above half coverage) raises Error.
        matte: (image, radius, eps) as for compute_mask_clicks -- the snapped selection comes back soft-edged.  cutout (with
        matte): as for compute_mask_clicks -- (coverage, rgba) comes back.  edge: as for compute_mask_clicks."""
        if clicks:
            return self.compute_mask_clicks(clicks, labels, None, out, refine_after, clean, lasso=mask, lasso_what=what,
                                            lasso_strength=strength, matte=matte, cutout=cutout, edge=edge)
        if labels or refine_after is not None:
            raise Error("snap_selection: labels and refine_after go with `clicks`")
        return Segmentation.compute_mask_batch([self], out=None if out is None else [out], clean=None if clean is None else [tuple(clean)],
                                               lasso=[mask], lasso_what=what, lasso_strength=strength,
                                               matte=None if matte is None else [tuple(matte)],
                                               cutout=None if cutout is None else [cutout],
                                               edge=None if edge is None else [edge])[0]

    def scribble(self, fg: np.ndarray, bg: Optional[np.ndarray] = None, clicks: int = 0, region: Optional[Region] = None,
                 out: Optional[np.ndarray] = None, clean=None, matte=None, cutout=None, edge=None):
        """Select by scribbling: fg, an (h, w) uint8 map of a stroke drawn over the object (a pixel belongs to it from 128 on),
        and optionally bg, a stroke over what the selection must leave out, are the prompt -- `clicks` foreground clicks (1 .. 8,
        0: the default 3) spread along fg and as many background clicks along bg, sampled on the GPU from the 256 x 256 low-res
        grid: the cell nearest the stroke's centroid, then farthest-point samples (dlimgedit.h, DLIMG_STROKE_MARK).  region: a
        box to go with them; clean, matte, cutout, edge and out as for compute_mask_clicks.  An empty stroke (no pixel from 128 on) raises
        Error."""
        marks = [(fg, 1, clicks)] + ([] if bg is None else [(bg, 0, clicks)])
        return self.compute_mask_clicks(None, None, region, out, None, clean, matte=matte, strokes=marks, cutout=cutout, edge=edge)

    @staticmethod
    def compute_mask_batch(segs: Sequence["Segmentation"], points: Optional[Sequence[Point]] = None,
                           regions: Optional[Sequence[Region]] = None, out: Optional[Sequence[np.ndarray]] = None,
                           clicks: Optional[Sequence[Sequence[Point]]] = None, labels=None, refine_after=None,
                           clean=None, grid=None, prior=None, prior_strength=0, lasso=None, lasso_what=0,
                           lasso_strength=0, matte=None, strokes=None, cutout=None, edge=None) -> list:
        """One single-mask query per entry of `segs`, decoded as one batch (table slot 14): a point each, a region each, or
        -- both given -- the box regions[i] refined by the foreground point points[i] in one prompt (SAM's combined prompt:
        point, top-left, bottom-right with labels 1, 2, 3; the mask is the decoder's output 0).
        `clicks` instead of `points`: prompt i is the clicks clicks[i] (1 .. 8) with labels[i] (1 / 0; None: foreground) and
        the box regions[i] (None: no box); prompts of different sizes may share the call (click_entries builds the lists).
        refine_after (with `clicks`): per prompt None, "each" or click counts, or one "each" for all -- refinement marks, see
        compute_mask_clicks.
        clean (either form): None, one (max_hole, max_island) pair for all prompts, or per prompt None / a pair -- clean-up
        marks, see compute_mask_clicks; a box-only call may carry them too.
        grid (either form): None, or per prompt None / (side, iou_permille, stability_permille) -- prompt i is a grid prompt,
        whose result is a label map (segment_everything); its point, clicks and region are not used (None will do), and with
        grid prompts alone neither `points` nor `regions` nor `clicks` is needed.
        prior (either form): None, or per prompt None / an (h, w) uint8 mask of the prompt's image -- prior marks, see
        compute_mask_clicks; prior_strength one int for all or one per prompt.  A box-only call may carry them too.
        lasso (either form): None, or per prompt None / an (h, w) uint8 selection -- lasso marks, see snap_selection; lasso_what
        and lasso_strength one int for all or one per prompt.  In a call with `points` or `clicks` those follow the derived
        click; a call without `points` may hold lasso-only prompts (regions[i] None) beside box-only ones, and with lasso
        prompts alone neither `points` nor `regions` is needed.
        matte (either form): None, or per prompt None / (image, radius, eps) -- matte marks, see compute_mask_clicks: the mask
        of such a prompt comes back as coverage 0 .. 255.
        strokes (with `clicks`, whose entries may then be None): None, or per prompt None / a list of (map, label, clicks) --
        stroke marks, see compute_mask_clicks and scribble.
        cutout (either form): None, or per prompt None / a radius / (radius, out) -- cut-out marks, see compute_mask_clicks: the
        result of such a prompt is (coverage, rgba) in place of the mask.
        edge (either form): None, or per prompt None / an int offset / (offset, feather, border) -- edge marks, see
        compute_mask_clicks; a box-only call may carry them too."""
        if strokes is not None and clicks is None:
            if points is not None:
                raise Error("compute_mask_batch: strokes go with `clicks` (whose entries may be None), not with `points`")
            clicks = [None] * len(segs)
        if refine_after is not None and clicks is None:
            raise Error("compute_mask_batch: refine_after goes with `clicks`")
        if clicks is not None:
            if points is not None:
                raise Error("compute_mask_batch: `points` or `clicks`, not both")
            if len(clicks) != len(segs):
                raise Error("compute_mask_batch: one list of clicks per segmentation")
            outs = [_mask_image(s.extent()) for s in segs] if out is None else list(out)
            assert len(outs) == len(segs) and all(o.dtype == np.uint8 and o.flags.c_contiguous for o in outs)
            cutouts = _checked_cutout(cutout, _checked_matte(matte, len(segs)), len(segs))
            entries = click_entries(clicks, labels, regions, refine_after, clean, grid, prior, prior_strength, lasso, lasso_what,
                                    lasso_strength, matte, strokes, cutouts, edge)
            out_of = {i: outs[j] for j, i in enumerate(entries.prompt_heads)}
            priors = _checked_prior(prior, prior_strength, len(segs))
            lassos = _checked_lasso(lasso, lasso_what, lasso_strength, len(segs))
            all_ptrs = _entry_pointers(segs, entries.heads, entries.regions, out_of, priors, lassos, _checked_matte(matte, len(segs)),
                                       _checked_strokes(strokes, len(segs)), cutouts)
            for sel, given in _entry_calls(entries):
                n, handles, p, r = _entry_arrays(segs, entries, sel, given)
                ptrs = (C.c_void_p * n)(*[all_ptrs[i] for i in sel])
                _check(api().get_segmentation_masks(handles, n, p, r, ptrs))
            return _with_cutouts(outs, cutouts)
        n = len(segs)
        outs = [_mask_image(s.extent()) for s in segs] if out is None else list(out)
        assert len(outs) == n and all(o.dtype == np.uint8 and o.flags.c_contiguous for o in outs)
        marks = _checked_clean(clean, n)
        grids = _checked_grid(grid, n)
        priors = _checked_prior(prior, prior_strength, n)
        lassos = _checked_lasso(lasso, lasso_what, lasso_strength, n)
        mattes = _checked_matte(matte, n)
        cutouts = _checked_cutout(cutout, mattes, n)
        edges = _checked_edge(edge, n)
        if any(m is not None for m in marks) or any(g is not None for g in grids) or any(q is not None for q in priors) \
                or any(q is not None for q in lassos) or any(q is not None for q in mattes) or any(q is not None for q in edges):
            if points is None and regions is None and any(g is None and q is None for g, q in zip(grids, lassos)):
                raise Error("compute_mask_batch: neither points nor regions given")
            heads, pts, regs = _marked_entries(n, points, regions, marks, grids, priors, lassos, mattes, cutouts, edges)
            m, handles, p, r = _marked_arrays(segs, heads, pts, regs)
            ptrs = (C.c_void_p * m)(*_entry_pointers(segs, heads, regs, {e: outs[h] for e, h in enumerate(heads) if h is not None}, priors,
                                                     lassos, mattes, None, cutouts))
            _check(api().get_segmentation_masks(handles, m, p, r, ptrs))
            return _with_cutouts(outs, cutouts)
        handles = (C.c_void_p * n)(*[s._handle for s in segs])
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        p = r = None
        if points is not None:
            p = (C.c_int * (2 * n))(*[v for q in points for v in (q.x, q.y)])
        if regions is not None:
            r = (C.c_int * (4 * n))(*[v for q in regions for v in (q.top_left.x, q.top_left.y, q.bottom_right.x,
                                                                  q.bottom_right.y)])
        _check(api().get_segmentation_masks(handles, n, p, r, ptrs))
        return outs

    def close(self) -> None:
        h, self._handle = self._handle, C.c_void_p()
        if h and _api is not None:
            _api.destroy_segmentation(h)

    def __del__(self):
        self.close()


def segment_objects(img: ImageView, env: Environment) -> np.ndarray:
    out = np.empty((img.extent.height, img.extent.width), dtype=np.uint8)
    v = img._c()
    _check(api().segment_objects(C.byref(v), out.ctypes.data, env.handle()))
    return out


# ---------------------------------------------------------------------------------------------
# extension entry points (include/dlimgedit/dlimgedit_amd.h)

STAGES = ("pre", "gemm", "layernorm", "attention_window", "attention_global", "encoder_other", "decoder", "post",
          "gemm_stats", "gemm_norm", "gemm_norm_gelu", "gemm_other", "gemm_patch", "gemm_proj", "gemm_fc2")


class ext:
    _sigs_done = False
    _hook_sigs_done = False

    @staticmethod
    def _apply(lib, sig):
        for name, (args, res) in sig.items():
            try:
                fn = getattr(lib, name)
            except AttributeError:           # an older library selected for an A/B (DLIMGEDIT_TUNING_LIB=<file>): the tools
                continue                     # that need the entry point fail when they call it; tests/test_abi.py checks them all
            fn.argtypes, fn.restype = args, res

    @classmethod
    def _l(cls):
        """The product library with the argument types of its extension entry points set."""
        lib = library()
        if not cls._sigs_done:
            vp, ci = C.c_void_p, C.c_int
            cls._apply(lib, {
                "dlimg_amd_device_count": ([], ci),
                "dlimg_amd_model_geometry": ([vp, C.POINTER(ci)], ci),
                "dlimg_amd_get_embedding": ([vp, vp], ci),
                "dlimg_amd_get_logits": ([vp, C.POINTER(ci), C.POINTER(ci), vp, vp], ci),
                "dlimg_amd_decoder_state": ([vp, C.POINTER(ci), vp, ci, C.c_char_p, ci], ci),
                "dlimg_amd_device_alloc": ([vp, C.c_size_t, C.POINTER(vp)], ci),
                "dlimg_amd_device_free": ([vp, vp], ci),
                "dlimg_amd_copy_to_device": ([vp, vp, vp, C.c_size_t], ci),
                "dlimg_amd_copy_to_host": ([vp, vp, vp, C.c_size_t], ci),
                "dlimg_amd_encode_and_mask": ([vp, C.POINTER(_ImageView), ci, C.POINTER(ci), C.POINTER(vp)], ci),
                "dlimg_amd_encode_only": ([vp, C.POINTER(_ImageView), ci], ci),
                "dlimg_amd_synchronize": ([vp], ci),
                "dlimg_amd_lane_count": ([vp], ci),
                "dlimg_amd_queue_config": ([vp, C.POINTER(ci)], ci),
                "dlimg_amd_image_memory": ([vp, C.c_size_t, C.POINTER(ci)], ci),
                "dlimg_amd_replica_count": ([vp], ci),
                "dlimg_amd_segmentation_device": ([vp, C.POINTER(ci), C.POINTER(ci)], ci),
                "dlimg_amd_get_segmentation_masks_device": ([C.POINTER(vp), ci, C.POINTER(ci), C.POINTER(ci), ci, vp,
                                                             C.POINTER(C.c_size_t)], ci),
                "dlimg_amd_set_profiling": ([vp, ci], ci),
                "dlimg_amd_take_stage_stats": ([vp, vp, vp, vp], ci),
                "dlimg_amd_birefnet_prepare_image": ([vp, ci, ci, ci, ci, vp, vp, vp], ci),
                "dlimg_amd_birefnet_process_mask": ([vp, ci, ci, vp], ci),
                "dlimg_amd_resize_mask": ([vp, ci, ci, ci, ci, ci, vp], ci),
            })
            cls._sigs_done = True
        return lib

    # (argument types, result type) of every hook of the test / tuning libraries, as include/dlimgedit/dlimgedit_amd_test.h
    # declares them; tests/test_abi.py holds its keys to HOOK_EXPORTS
    _vp, _ci, _cf, _ip, _fp = C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_float)
    _HOOK_SIGS = {
        "dlimg_amd_test_mask_pieces": ([_ci, C.POINTER(C.c_longlong), C.c_longlong, C.POINTER(C.c_longlong), _ci,
                                       C.POINTER(C.c_longlong), _ci, _ip], _ci),
        "dlimg_amd_test_plan_steps": ([_ci, _ip, _ip, _ip, _ci, _ci, _ci, _ci, _ip, _ip, _ci], _ci),
        "dlimg_amd_test_parse_cpu_list": ([C.c_char_p, _ip, _ci], _ci),
        "dlimg_amd_test_preprocess": ([_vp, _ci, _ci, _ci, _ci, _vp], _ci),
        "dlimg_amd_test_postprocess": ([_vp, _ci, _vp, _ci, _ci, _vp], _ci),
        "dlimg_amd_test_postprocess_batch": ([_vp, _ci, _ci, _ci, _vp], _ci),
        "dlimg_amd_test_force_gemm_tile": ([_ci], _ci),
        "dlimg_amd_test_force_gemm_consumer_tile": ([_ci], _ci),
        "dlimg_amd_test_gemm": ([_ci, _ci, _ci, _vp, _vp, _vp, _vp, _ci, _ci, _vp, _vp], _ci),
        "dlimg_amd_test_gemm_ln": ([_ci, _ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _ci, _vp, _vp, _vp, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_gemm_tile_shape": ([_ci, _ip, _ip], _ci),
        "dlimg_amd_test_lane_worker": ([_ci, _ci, _vp], _ci),
        "dlimg_amd_test_gemm_stream": ([_ci, _ci, _ci, _vp, _vp, _vp, _vp, _vp, _ci, _vp, _vp, _vp, _vp], _ci),
        "dlimg_amd_test_layernorm": ([_vp, _vp, _vp, _cf, _ci, _ci, _ci, _vp, _vp], _ci),
        "dlimg_amd_test_attention": ([_ci, _vp, _vp, _vp, _vp, _ci, _ci, _ci, _vp], _ci),
        "dlimg_amd_test_resize": ([_vp, _ci, _ci, _ci, _ci, _ci, _ci, _vp], _ci),
        "dlimg_amd_test_decode": ([_vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp], _ci),
        "dlimg_amd_test_decode_prompts": ([_vp, _ci, _vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _ci, C.c_char_p, _ci], _ci),
        "dlimg_amd_test_encoder_state": ([_vp, C.POINTER(_ImageView), _ci, _ci, _vp, C.c_longlong, C.c_char_p, _ci, _ci, _vp,
                                          C.c_longlong, C.c_char_p, _ci], _ci),
        "dlimg_amd_test_neck_conv1x1_ln": ([_vp, _ci, _ci, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_neck_conv3x3_ln": ([_vp, _ci, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_mask_cleanup": ([C.POINTER(C.c_void_p), _ip, _ip, _ip, _ip, _ci], _ci),
        "dlimg_amd_test_grid_kernels": ([_fp, _ci, _fp, _ci, _ci, _ci, _ci, _ci, _ci, _ip, _ci, _ci, C.POINTER(C.c_int32), _fp, _vp,
                                         _ip, _ip, _ip, _ci, _fp], _ci),
        "dlimg_amd_test_prior_plane": ([_vp, _ci, _ci, _ci, _ci, _ci, _fp, _ip, _ci, _fp], _ci),
        "dlimg_amd_test_lasso_derive": ([_vp, _ci, _ci, _ci, _ci, C.POINTER(C.c_int32), _ip, _ci, _fp], _ci),
        "dlimg_amd_test_hq_mask_path": ([_vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _cf, _vp, _ci, _ip, _vp, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_upscale_logits": ([_vp, _ci, _vp, _vp, _vp, _vp, _cf, _vp, _vp, _vp, _ci, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_hq_features_finish": ([_vp, _vp, _vp, _vp, _vp, _ip], _ci),
        "dlimg_amd_test_hq_branch": ([_vp, _ci, _vp, _ci, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], _ci),
        "dlimg_amd_test_layernorm_rows": ([_vp, _vp, _vp, _cf, _ci, _ci, _ci, _ci, _ci, _vp, _vp, _ip, _ip], _ci),
        "dlimg_amd_test_elementwise": ([_ci, _vp, _vp, _vp, C.c_longlong, C.c_longlong, _vp, _vp, _ip], _ci),
        "dlimg_amd_bench_attention": ([_ci, _ci, _ci, _ci, _ci, C.POINTER(C.c_double)], _ci),
        "dlimg_amd_bench_prepost": ([_ci, _ci, _ci, C.POINTER(C.c_double), C.POINTER(C.c_double)], _ci),
        "dlimg_amd_bench_gemm": ([_ci, _ci, _ci, _ci, _ci, _ci, C.POINTER(C.c_double)], _ci),
        "dlimg_amd_bench_gemm_streams": ([_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, C.POINTER(C.c_double)], _ci),
        "dlimg_amd_bench_gemm_stamps": ([_ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, _ci, C.POINTER(C.c_double), _vp, _ci], _ci),
    }

    @classmethod
    def _h(cls):
        """The library with the test / benchmark hooks (hooks_library()), their argument types set."""
        lib = hooks_library()
        if not cls._hook_sigs_done:
            cls._apply(lib, cls._HOOK_SIGS)
            cls._hook_sigs_done = True
        return lib

    # entry points of the product library (include/dlimgedit/dlimgedit_amd.h; csrc/exports.map)
    EXPORTS = (
               "dlimg_amd_device_count", "dlimg_amd_model_geometry", "dlimg_amd_get_embedding",
               "dlimg_amd_get_logits", "dlimg_amd_decoder_state", "dlimg_amd_device_alloc", "dlimg_amd_device_free",
               "dlimg_amd_copy_to_device", "dlimg_amd_copy_to_host", "dlimg_amd_encode_and_mask",
               "dlimg_amd_encode_only", "dlimg_amd_synchronize", "dlimg_amd_lane_count", "dlimg_amd_queue_config",
               "dlimg_amd_image_memory",
               "dlimg_amd_replica_count", "dlimg_amd_segmentation_device", "dlimg_amd_get_segmentation_masks_device",
               "dlimg_amd_set_profiling", "dlimg_amd_take_stage_stats", "dlimg_amd_birefnet_prepare_image",
               "dlimg_amd_birefnet_process_mask", "dlimg_amd_resize_mask")
    # hooks of the test / tuning libraries (include/dlimgedit/dlimgedit_amd_test.h)
    HOOK_EXPORTS = (
               "dlimg_amd_test_mask_pieces", "dlimg_amd_test_plan_steps", "dlimg_amd_test_parse_cpu_list", "dlimg_amd_test_preprocess",
               "dlimg_amd_test_postprocess", "dlimg_amd_test_postprocess_batch", "dlimg_amd_test_force_gemm_tile",
               "dlimg_amd_test_force_gemm_consumer_tile", "dlimg_amd_test_gemm", "dlimg_amd_test_gemm_ln",
               "dlimg_amd_test_lane_worker", "dlimg_amd_test_gemm_stream", "dlimg_amd_test_layernorm",
               "dlimg_amd_test_attention", "dlimg_amd_test_resize", "dlimg_amd_test_decode", "dlimg_amd_test_decode_prompts",
               "dlimg_amd_test_encoder_state",
               "dlimg_amd_test_neck_conv1x1_ln", "dlimg_amd_test_neck_conv3x3_ln", "dlimg_amd_test_mask_cleanup",
               "dlimg_amd_test_grid_kernels", "dlimg_amd_test_prior_plane", "dlimg_amd_test_lasso_derive",
               "dlimg_amd_test_hq_mask_path", "dlimg_amd_test_upscale_logits", "dlimg_amd_test_hq_features_finish",
               "dlimg_amd_test_hq_branch", "dlimg_amd_test_layernorm_rows", "dlimg_amd_test_elementwise",
               "dlimg_amd_bench_attention",
               "dlimg_amd_bench_prepost", "dlimg_amd_bench_gemm", "dlimg_amd_bench_gemm_streams",
               "dlimg_amd_bench_gemm_stamps", "dlimg_amd_test_gemm_tile_shape")

    @staticmethod
    def _ptr(a: Optional[np.ndarray]):
        return None if a is None else a.ctypes.data

    @classmethod
    def device_count(cls) -> int:
        return cls._l().dlimg_amd_device_count()

    @classmethod
    def model_geometry(cls, env: Environment) -> Tuple[int, int, int, int]:
        out = (C.c_int * 4)()
        _check(cls._l().dlimg_amd_model_geometry(env.handle(), out))
        return tuple(out)

    @classmethod
    def get_embedding(cls, seg: Segmentation) -> np.ndarray:
        out = np.empty((4096, 256), dtype=np.float32)
        _check(cls._l().dlimg_amd_get_embedding(seg._handle, out.ctypes.data))
        return out

    @classmethod
    def get_logits(cls, seg: Segmentation, point: Optional[Point] = None, region: Optional[Region] = None):
        logits = np.empty((4, 256, 256), dtype=np.float32)
        iou = np.empty(4, dtype=np.float32)
        p = (C.c_int * 2)(point.x, point.y) if point is not None else None
        r = (C.c_int * 4)(region.top_left.x, region.top_left.y, region.bottom_right.x, region.bottom_right.y) \
            if region is not None else None
        _check(cls._l().dlimg_amd_get_logits(seg._handle, p, r, logits.ctypes.data, iou.ctypes.data))
        return logits, iou

    @classmethod
    def decoder_state(cls, seg: Segmentation, point: Point):
        """Diagnostic: {name: array} of the decoder's token-side workspaces after decoding `point`."""
        buf = C.create_string_buffer(1024)
        _check(cls._l().dlimg_amd_decoder_state(seg._handle, (C.c_int * 2)(point.x, point.y), None, 0, buf, 1024))
        parts = [(n, int(c)) for n, c in (item.split(":") for item in buf.value.decode().strip(",").split(","))]
        out = np.empty(sum(c for _, c in parts), dtype=np.float32)
        _check(cls._l().dlimg_amd_decoder_state(seg._handle, (C.c_int * 2)(point.x, point.y), out.ctypes.data, out.size, None, 0))
        res, off = {}, 0
        for n, c in parts:
            res[n] = out[off:off + c]
            off += c
        return res

    @classmethod
    def mask_pieces(cls, mask_bytes, extra_bytes: int = 0):
        """Host logic of the mask transfer (no GPU needed): (piece end offsets, [(piece, mask, staging offset, offset in the
        mask, bytes)])."""
        n = len(mask_bytes)
        sizes = (C.c_longlong * max(1, n))(*mask_bytes)
        ends = (C.c_longlong * 8)()
        cap = 8 * (n + 1)
        copies = (C.c_longlong * (5 * cap))()
        pieces = C.c_int(0)
        got = cls._h().dlimg_amd_test_mask_pieces(n, sizes, extra_bytes, ends, 8, copies, cap, C.byref(pieces))
        if got < 0:
            _check_hook(1)
        return [ends[i] for i in range(pieces.value)], [tuple(copies[5 * k + j] for j in range(5)) for k in range(got)]

    @classmethod
    def plan_steps(cls, passes_in_flight, images_in_flight, cursor: int, pending: int, width: int, depth: int, all_: bool):
        """Host logic of the device-step queue (no GPU needed): returns (passes [(lane, images)], new passes in flight, new
        images in flight, new cursor)."""
        lanes = len(passes_in_flight)
        p = (C.c_int * lanes)(*passes_in_flight)
        i = (C.c_int * lanes)(*images_in_flight)
        cur = C.c_int(cursor)
        cap = pending + lanes + 1
        out_lane, out_images = (C.c_int * cap)(), (C.c_int * cap)()
        n = cls._h().dlimg_amd_test_plan_steps(lanes, p, i, C.byref(cur), pending, width, depth, int(all_), out_lane, out_images, cap)
        if n < 0:
            _check_hook(1)
        return [(out_lane[k], out_images[k]) for k in range(n)], list(p), list(i), cur.value

    @classmethod
    def parse_cpu_list(cls, text: str) -> list:
        """Host logic (no GPU needed): sysfs cpulist text -> CPU indices, as the multi-GPU helper threads' binding reads it."""
        out = (C.c_int * 4096)()
        n = cls._h().dlimg_amd_test_parse_cpu_list(text.encode(), out, 4096)
        if n < 0:
            _check_hook(1)
        return list(out[:n])

    # -- benchmark path
    @classmethod
    def device_alloc(cls, env, nbytes: int) -> int:
        out = C.c_void_p()
        _check(cls._l().dlimg_amd_device_alloc(env.handle(), nbytes, C.byref(out)))
        return out.value

    @classmethod
    def device_free(cls, env, ptr: int) -> None:
        _check(cls._l().dlimg_amd_device_free(env.handle(), ptr))

    @classmethod
    def copy_to_device(cls, env, dst: int, src: np.ndarray) -> None:
        src = np.ascontiguousarray(src)
        _check(cls._l().dlimg_amd_copy_to_device(env.handle(), dst, src.ctypes.data, src.nbytes))

    @classmethod
    def copy_to_host(cls, env, dst: np.ndarray, src: int) -> None:
        _check(cls._l().dlimg_amd_copy_to_host(env.handle(), dst.ctypes.data, src, dst.nbytes))

    @staticmethod
    def device_views(ptrs, width, height, channels=Channels.rgba, stride=None):
        """Views of device-resident images for encode_and_mask / encode_only.  width, height, channels and stride are one
        value for all views or one per view; stride defaults to packed rows.  Any size: the library resamples a view
        whose longest side is not 1024 on the device, exactly as process() resamples a host image of that size."""
        n = len(ptrs)

        def per_view(value):
            return list(value) if isinstance(value, (list, tuple)) else [value] * n

        ws, hs, cs, ss = per_view(width), per_view(height), per_view(channels), per_view(stride)
        return (_ImageView * n)(*[_ImageView(ws[i], hs[i], int(cs[i]), ws[i] * count(cs[i]) if ss[i] is None else ss[i], ptrs[i])
                                  for i in range(n)])

    @classmethod
    def encode_and_mask(cls, env, views, points, mask_ptrs) -> None:
        """Queues one request per view: encode the device-resident image, decode points[i] (pixels of the view's own
        width x height) and write the mask, width x height bytes, to the device buffer mask_ptrs[i].  Views may have any
        size and differ from each other; requests of different sizes share a pass as requests of one size do.  Returns once
        the requests are queued; synchronize() waits for the masks and reports what failed."""
        n = len(views)
        p = (C.c_int * (2 * n))(*[v for q in points for v in (q.x, q.y)])
        m = (C.c_void_p * n)(*mask_ptrs)
        _check(cls._l().dlimg_amd_encode_and_mask(env.handle(), views, n, p, m))

    @classmethod
    def encode_only(cls, env, views) -> None:
        """Encodes the device-resident images of `views` (any size, see device_views) in one pass; enqueues only."""
        _check(cls._l().dlimg_amd_encode_only(env.handle(), views, len(views)))

    @classmethod
    def synchronize(cls, env) -> None:
        _check(cls._l().dlimg_amd_synchronize(env.handle()))

    @classmethod
    def lane_count(cls, env) -> int:
        return cls._l().dlimg_amd_lane_count(env.handle())

    @classmethod
    def queue_config(cls, env) -> dict:
        """Effective settings of the step queue behind encode_and_mask, as the library clamped them."""
        out = (C.c_int * 6)()
        _check(cls._l().dlimg_amd_queue_config(env.handle(), out))
        return {"coalesce": out[0], "step_depth": out[1], "lanes": out[2], "lanes_in_use": out[3],
                "one_image_passes": out[4], "one_image_passes_alone": out[5]}

    @classmethod
    def image_memory_is_pinned(cls, array: np.ndarray) -> bool:
        """True when the array's bytes lie in pinned image memory of the library (read / written in place by the GPU)."""
        out = C.c_int(0)
        _check(cls._l().dlimg_amd_image_memory(array.ctypes.data, array.nbytes, C.byref(out)))
        return bool(out.value)

    @classmethod
    def replica_count(cls, env) -> int:
        return cls._l().dlimg_amd_replica_count(env.handle())

    @classmethod
    def segmentation_device(cls, seg) -> Tuple[int, int]:
        """(replica index in the environment's device list, HIP device index) holding the embedding."""
        r, d = C.c_int(), C.c_int()
        _check(cls._l().dlimg_amd_segmentation_device(seg._handle, C.byref(r), C.byref(d)))
        return r.value, d.value

    @classmethod
    def compute_mask_batch_device(cls, segs, dev_out: int, points=None, regions=None, root_device: int = 0, clicks=None,
                                  labels=None, refine_after=None, clean=None, grid=None, edge=None) -> list:
        """Device-output form of Segmentation.compute_mask_batch (points, regions or both, or clicks / labels / regions, as
        there): masks land tightly packed at `dev_out` (a device pointer on HIP device `root_device`), wherever their
        embeddings live; returns the byte offset of every mask.  refine_after, clean, grid, edge: as there (a grid prompt's
        label map is delivered as a mask is; an edge mark needs no pointer, so this form serves it)."""
        if refine_after is not None and clicks is None:
            raise Error("compute_mask_batch_device: refine_after goes with `clicks`")
        if clicks is not None:
            if points is not None:
                raise Error("compute_mask_batch_device: `points` or `clicks`, not both")
            if len(clicks) != len(segs):
                raise Error("compute_mask_batch_device: one list of clicks per segmentation")
            entries = click_entries(clicks, labels, regions, refine_after, clean, grid, edge=edge)
            calls = _entry_calls(entries)
            if len(calls) > 1:      # one-click prompts with and without a box: a call each, so that the masks stay in order
                calls = [([i], entries.regions[i] != EMPTY_REGION) for i in range(len(entries.heads))]
            result, base = [], 0
            for sel, given in calls:
                n, handles, p, r = _entry_arrays(segs, entries, sel, given)
                offsets = (C.c_size_t * n)()
                _check(cls._l().dlimg_amd_get_segmentation_masks_device(handles, n, p, r, root_device, dev_out + base, offsets))
                result += [base + offsets[k] for k, i in enumerate(sel) if entries.heads[i] is not None]
                e = segs[entries.heads[sel[0]]].extent()
                base += e.width * e.height if len(calls) > 1 else 0
            return result
        n = len(segs)
        marks = _checked_clean(clean, n)
        grids = _checked_grid(grid, n)
        edges = _checked_edge(edge, n)
        if any(m is not None for m in marks) or any(g is not None for g in grids) or any(q is not None for q in edges):
            if points is None and regions is None and any(g is None for g in grids):
                raise Error("compute_mask_batch_device: neither points nor regions given")
            heads, pts, regs = _marked_entries(n, points, regions, marks, grids, edge=edges)
            m, handles, p, r = _marked_arrays(segs, heads, pts, regs)
            offsets = (C.c_size_t * m)()
            _check(cls._l().dlimg_amd_get_segmentation_masks_device(handles, m, p, r, root_device, dev_out, offsets))
            return [offsets[k] for k, h in enumerate(heads) if h is not None]
        handles = (C.c_void_p * n)(*[s._handle for s in segs])
        p = r = None
        if points is not None:
            p = (C.c_int * (2 * n))(*[v for q in points for v in (q.x, q.y)])
        if regions is not None:
            r = (C.c_int * (4 * n))(*[v for q in regions for v in (q.top_left.x, q.top_left.y, q.bottom_right.x,
                                                                  q.bottom_right.y)])
        offsets = (C.c_size_t * n)()
        _check(cls._l().dlimg_amd_get_segmentation_masks_device(handles, n, p, r, root_device, dev_out, offsets))
        return list(offsets)

    @classmethod
    def set_profiling(cls, env, on: bool) -> None:
        _check(cls._l().dlimg_amd_set_profiling(env.handle(), int(on)))

    @classmethod
    def take_stage_stats(cls, env) -> dict:
        n = len(STAGES)
        ms, work, launches = (C.c_double * n)(), (C.c_double * n)(), (C.c_long * n)()
        _check(cls._l().dlimg_amd_take_stage_stats(env.handle(), ms, work, launches))
        return {s: {"ms": ms[i], "work": work[i], "launches": launches[i]} for i, s in enumerate(STAGES)}

    # -- single-kernel hooks
    @classmethod
    def test_preprocess(cls, pixels: np.ndarray, channels: Channels, stride: Optional[int] = None) -> np.ndarray:
        h, w = pixels.shape[:2]
        if stride is None:
            pixels = np.ascontiguousarray(pixels)
            stride = w * count(channels)
        out = np.empty((4096, 768), dtype=np.float16)
        _check_hook(cls._h().dlimg_amd_test_preprocess(pixels.ctypes.data, w, h, stride, int(channels), out.ctypes.data))
        return out

    @classmethod
    def test_postprocess(cls, planes: np.ndarray, out_w: int, out_h: int, iou: Optional[np.ndarray] = None) -> np.ndarray:
        planes = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 256, 256)
        out = np.empty((out_h, out_w), dtype=np.uint8)
        iou = None if iou is None else np.ascontiguousarray(iou, dtype=np.float32)
        _check_hook(cls._h().dlimg_amd_test_postprocess(planes.ctypes.data, planes.shape[0], cls._ptr(iou), out_w, out_h,
                                                   out.ctypes.data))
        return out

    @classmethod
    def test_postprocess_batch(cls, planes: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
        """One launch for all planes (one mask each): the batched form of the post-processing kernel."""
        planes = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, 256, 256)
        out = np.empty((planes.shape[0], out_h, out_w), dtype=np.uint8)
        _check_hook(cls._h().dlimg_amd_test_postprocess_batch(planes.ctypes.data, planes.shape[0], out_w, out_h, out.ctypes.data))
        return out

    @classmethod
    def force_gemm_tile(cls, tile: int = -1, consumer_tile: int = -1) -> None:
        """Tile configuration the GEMM test hooks use wherever it fits (-1: the product's own choice); consumer_tile: a
        separate one for the LayerNorm-folded consumer of test_gemm_ln.  One forced tile is not replaced where it does not fit: a
        ping-pong tile (9, 10, 11) for an f16-only result with a residual, whose f16-rows epilogue would drop the residual --
        that launch raises Error."""
        _check_hook(cls._h().dlimg_amd_test_force_gemm_tile(int(tile)))
        _check_hook(cls._h().dlimg_amd_test_force_gemm_consumer_tile(int(consumer_tile)))

    @classmethod
    def gemm_tile_shape(cls, tile: int) -> Tuple[int, int]:
        """(bm, bn) of tile configuration `tile`, from k::kGemmTiles (csrc/gemm_plan.hpp)."""
        bm, bn = C.c_int(0), C.c_int(0)
        _check_hook(cls._h().dlimg_amd_test_gemm_tile_shape(int(tile), C.byref(bm), C.byref(bn)))
        return bm.value, bn.value

    @classmethod
    def test_gemm(cls, A: np.ndarray, W: np.ndarray, bias=None, resid=None, act: int = 0, want_f16: bool = False,
                  want_f32: bool = True):
        """want_f32=False with want_f16=True: the launch gets out_h only (the f16-only epilogues); returns the f16 result."""
        assert want_f32 or want_f16, "no output asked for"
        A = np.ascontiguousarray(A, dtype=np.float16)
        W = np.ascontiguousarray(W, dtype=np.float16)
        M, K = A.shape
        N = W.shape[0]
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        resid = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
        out32 = np.empty((M, N), dtype=np.float32) if want_f32 else None
        out16 = np.empty((M, N), dtype=np.float16) if want_f16 else None
        _check_hook(cls._h().dlimg_amd_test_gemm(M, N, K, A.ctypes.data, W.ctypes.data, cls._ptr(bias), cls._ptr(resid),
                                            0 if resid is None else resid.shape[0], act, cls._ptr(out32),
                                            cls._ptr(out16)))
        if not want_f32:
            return out16
        return (out32, out16) if want_f16 else out32

    @classmethod
    def test_gemm_ln(cls, A1, W1, bias1, resid, W2, gamma, beta, bias2, eps: float, act: int = 0, consumer_out: str = "f32",
                     operands: bool = False):
        """x = A1.W1^T + bias1 + resid; y = act(LayerNorm(x; gamma, beta).W2^T + bias2), with the LayerNorm folded into
        the second GEMM the way SamWeights does it (csrc/sam_model.cpp, Loader::linear_ln_h).  Returns (x, x as f16, y).
        consumer_out: "f32" (y fp32), "f16" (the consumer gets out_h only, as qkv and fc1 do in the product; y f16) or "both"
        (y = (fp32, f16)).  Then additionally returns the producer's row statistics [D / block, M, 2] = (sum, sum of squared
        deviations from the block mean) per block of `block` columns, and with operands=True the consumer's own operands
        {"wg": f16 scaled weight, "colsum": fp32, "bias": fp32} as passed to the kernel."""
        assert consumer_out in ("f32", "f16", "both"), consumer_out
        A1 = np.ascontiguousarray(A1, dtype=np.float16)
        W1 = np.ascontiguousarray(W1, dtype=np.float16)
        M, K1 = A1.shape
        D = W1.shape[0]
        W2 = np.asarray(W2, dtype=np.float32)
        N = W2.shape[0]
        wg = np.ascontiguousarray((W2 * np.asarray(gamma, np.float32)[None, :]).astype(np.float16))
        colsum = np.ascontiguousarray(wg.astype(np.float64).sum(axis=1).astype(np.float32))
        b2 = np.ascontiguousarray((np.asarray(bias2, np.float64) + W2.astype(np.float64) @ np.asarray(beta, np.float64))
                                  .astype(np.float32))
        bias1 = None if bias1 is None else np.ascontiguousarray(bias1, dtype=np.float32)
        resid = None if resid is None else np.ascontiguousarray(resid, dtype=np.float32)
        x = np.empty((M, D), dtype=np.float32)
        xh = np.empty((M, D), dtype=np.float16)
        y = np.empty((M, N), dtype=np.float32) if consumer_out != "f16" else None
        yh = np.empty((M, N), dtype=np.float16) if consumer_out != "f32" else None
        stats = np.empty((M * 48,), dtype=np.float32)
        block = C.c_int(0)
        _check_hook(cls._h().dlimg_amd_test_gemm_ln(M, D, K1, N, A1.ctypes.data, W1.ctypes.data, cls._ptr(bias1),
                                               cls._ptr(resid), wg.ctypes.data, colsum.ctypes.data, b2.ctypes.data,
                                               eps, act, x.ctypes.data, xh.ctypes.data, cls._ptr(y), cls._ptr(yh),
                                               stats.ctypes.data, C.byref(block)))
        if consumer_out == "f32" and not operands:
            return x, xh, y
        out = y if consumer_out == "f32" else yh if consumer_out == "f16" else (y, yh)
        st = stats[:(D // block.value) * M * 2].reshape(D // block.value, M, 2).copy()
        if operands:
            return x, xh, out, st, {"wg": wg, "colsum": colsum, "bias": b2}
        return x, xh, out, st

    @classmethod
    def test_lane_worker(cls, tasks: int, sleep_us: int = 0):
        """Runs the LaneWorker host-logic check; returns the order the tasks ran in (tasks + 1 entries when all ran)."""
        order = np.full(tasks + 1, -1, dtype=np.int32)
        ran = cls._h().dlimg_amd_test_lane_worker(tasks, sleep_us, order.ctypes.data)
        if ran < 0:
            _check_hook(1)
        return order[:ran].tolist()

    @classmethod
    def test_gemm_stream(cls, A, W, bias, resid_hi, resid_lo, pair: bool):
        """One stream-writing GEMM with row statistics; returns (x fp32 or None, hi, lo or None, stats[M, 48])."""
        A = np.ascontiguousarray(A, dtype=np.float16)
        W = np.ascontiguousarray(W, dtype=np.float16)
        M, K = A.shape
        D = W.shape[0]
        bias = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        resid_hi = None if resid_hi is None else np.ascontiguousarray(resid_hi, dtype=np.float16)
        resid_lo = None if resid_lo is None else np.ascontiguousarray(resid_lo, dtype=np.float16)
        x = None if pair else np.empty((M, D), dtype=np.float32)
        hi = np.empty((M, D), dtype=np.float16)
        lo = np.empty((M, D), dtype=np.float16) if pair else None
        stats = np.empty((M * 48,), dtype=np.float32)
        _check_hook(cls._h().dlimg_amd_test_gemm_stream(M, D, K, A.ctypes.data, W.ctypes.data, cls._ptr(bias), cls._ptr(resid_hi),
                                                   cls._ptr(resid_lo), int(pair), cls._ptr(x), hi.ctypes.data,
                                                   cls._ptr(lo), stats.ctypes.data))
        return x, hi, lo, stats

    @classmethod
    def test_layernorm(cls, x, w, b, eps: float, act: int = 0):
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        rows, dim = x.shape
        o32 = np.empty_like(x)
        o16 = np.empty(x.shape, dtype=np.float16)
        _check_hook(cls._h().dlimg_amd_test_layernorm(x.ctypes.data, w.ctypes.data, b.ctypes.data, eps, rows, dim, act,
                                                 o32.ctypes.data, o16.ctypes.data))
        return o32, o16

    @classmethod
    def test_mask_cleanup(cls, masks, max_hole, max_island, shapes=None) -> list:
        """The mask clean-up kernels alone (dlimg_amd_test_mask_cleanup): `masks`, (h, w) uint8 arrays of 0 / 255 of
        possibly different sizes, as ONE k::mask_cleanup call on the default device; max_hole / max_island: one int for all or
        one per mask.  Returns the cleaned masks (the inputs are left alone).  For the launcher's refusals a mask may be None
        (a null pointer) and shapes[i] = (h, w) may claim an extent of its own; a refusal raises Error."""
        n = len(masks)
        hole = [int(max_hole)] * n if isinstance(max_hole, (int, np.integer)) else [int(v) for v in max_hole]
        isle = [int(max_island)] * n if isinstance(max_island, (int, np.integer)) else [int(v) for v in max_island]
        if len(hole) != n or len(isle) != n:
            raise Error("test_mask_cleanup: one threshold for all masks or one per mask")
        outs = [None if m is None else np.array(m, dtype=np.uint8, order="C", copy=True) for m in masks]
        if shapes is None:
            if any(o is None or o.ndim != 2 for o in outs):
                raise Error("test_mask_cleanup: a mask is an (h, w) array; a None mask needs `shapes`")
            shapes = [o.shape for o in outs]
        ptrs = (C.c_void_p * n)(*[None if o is None else o.ctypes.data for o in outs])
        w = (C.c_int * n)(*[int(s[1]) for s in shapes])
        h = (C.c_int * n)(*[int(s[0]) for s in shapes])
        _check_hook(cls._h().dlimg_amd_test_mask_cleanup(ptrs, w, h, (C.c_int * n)(*hole), (C.c_int * n)(*isle), n))
        return outs

    @classmethod
    def test_grid_kernels(cls, planes4: np.ndarray, out_w: int, out_h: int, pre_w: int, pre_h: int, kept=None, iou4=None,
                          iou_permille: int = 0, stability_permille: int = 0, cull: bool = True, want_store: bool = False,
                          time_iters: int = 0):
        """The label-map kernels alone (dlimg_amd_test_grid_kernels): planes4 [P, 4, 256, 256] fp32 as a decode leaves them,
        harvested in chunks of 16 prompts; then the candidates `kept` (label order; candidate c = 3 * prompt + plane - 1) are
        painted into an (out_h, out_w) map for an image encoded at pre_w x pre_h -- or, with kept None, the candidates the
        library's own selection keeps from the records and iou4 [P, 4] with the two thresholds.
        -> (records int32 [3 P, 8], map uint8, kept list, guard bytes intact, store [3 P, 256, 256] or None); with time_iters > 0
        the last element is instead (ms of one harvest of all candidates, ms of one paint launch), each the mean of time_iters
        repetitions between two events."""
        planes4 = np.ascontiguousarray(planes4, np.float32)
        P = planes4.shape[0]
        assert planes4.shape == (P, 4, 256, 256)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        iou = None if iou4 is None else np.ascontiguousarray(iou4, np.float32)
        assert iou is None or iou.shape == (P, 4)
        kin = None if kept is None else np.ascontiguousarray(kept, np.int32)
        records = np.zeros((3 * P, 8), np.int32)
        store = np.zeros((3 * P, 256, 256), np.float32) if want_store else None
        out = np.zeros((out_h, out_w), np.uint8)
        kout = np.zeros(255, np.int32)
        nk, ok = C.c_int(0), C.c_int(0)
        ms = (C.c_float * 2)(0.0, 0.0)
        _check_hook(cls._h().dlimg_amd_test_grid_kernels(
            planes4.ctypes.data_as(fp), P, None if iou is None else iou.ctypes.data_as(fp), out_w, out_h, pre_w, pre_h,
            iou_permille, stability_permille, None if kin is None else kin.ctypes.data_as(ip), -1 if kin is None else len(kin),
            int(cull), records.ctypes.data_as(C.POINTER(C.c_int32)), None if store is None else store.ctypes.data_as(fp),
            out.ctypes.data, kout.ctypes.data_as(ip), C.byref(nk), C.byref(ok), int(time_iters), ms))
        return records, out, [int(v) for v in kout[:nk.value]], bool(ok.value), (store if time_iters <= 0 else (ms[0], ms[1]))

    @classmethod
    def test_prior_plane(cls, mask: np.ndarray, pre_w: int, pre_h: int, strength_milli: int, time_iters: int = 0):
        """The prior-plane kernel alone (dlimg_amd_test_prior_plane): mask (h, w) uint8, of an image that was encoded at
        pre_w x pre_h, through ONE k::mask_prior launch on the default device, with guard bytes around the plane and around the
        mask's device copy.  -> (plane float32 [256, 256], guard bytes intact); with time_iters > 0 a third element, the
        milliseconds of one launch (the mean of time_iters repetitions between two events).  A refusal of the launcher raises
        Error."""
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.ndim == 2
        h, w = mask.shape
        plane = np.zeros((256, 256), np.float32)
        ok, ms = C.c_int(0), C.c_float(0.0)
        _check_hook(cls._h().dlimg_amd_test_prior_plane(mask.ctypes.data, w, h, int(pre_w), int(pre_h), int(strength_milli),
                                                        plane.ctypes.data_as(C.POINTER(C.c_float)), C.byref(ok), int(time_iters),
                                                        C.byref(ms)))
        return (plane, bool(ok.value)) if time_iters <= 0 else (plane, bool(ok.value), float(ms.value))

    @classmethod
    def test_lasso_derive(cls, mask: np.ndarray, pre_w: int, pre_h: int, time_iters: int = 0):
        """The lasso derivation alone (dlimg_amd_test_lasso_derive): mask (h, w) uint8, of an image that was encoded at
        pre_w x pre_h, through k::mask_prior, the two launches of k::lasso_derive and the host's fold, with guard bytes around
        every device buffer.  -> (record int32 [8] = inside cells, box x0, y0, x1, y1, click x, click y, d2; guard bytes
        intact); with time_iters > 0 a third element, the milliseconds of one derivation (both launches; the mean of
        time_iters repetitions between two events).  A refusal of a launcher raises Error."""
        mask = np.ascontiguousarray(mask, np.uint8)
        assert mask.ndim == 2
        h, w = mask.shape
        record = np.zeros(8, np.int32)
        ok, ms = C.c_int(0), C.c_float(0.0)
        _check_hook(cls._h().dlimg_amd_test_lasso_derive(mask.ctypes.data, w, h, int(pre_w), int(pre_h),
                                                         record.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ok), int(time_iters),
                                                         C.byref(ms)))
        return (record, bool(ok.value)) if time_iters <= 0 else (record, bool(ok.value), float(ms.value))

    @classmethod
    def test_hq_mask_path(cls, U, weights, eps: float, features, feat_index, hyper_hq, logits_in=None, want_h: bool = True,
                          prompts: Optional[int] = None):
        """k::hq_mask_path alone (dlimg_amd_test_hq_mask_path), ONE launcher call on host operands with guard bytes around every
        device buffer.  U (P, 256, 256, 32) float16; weights = (conv1_w (9, 64, 32) f16, conv1_b, ln_w, ln_b (64,), conv2_w
        (9, 32, 64) f16, conv2_b (32,)); features (n, 256, 256, 32) float32, prompt i taking features[feat_index[i]] (-1: a null
        pointer); hyper_hq (P, 32); logits_in (P, 4, 256, 256), zeros when omitted.  prompts: the P the launcher is given, when it
        is not len(U) (the refusals).  -> (logits (P, 4, 256, 256) float32, H (P, 256, 256, 64) float16 or None, guard bytes
        intact).  A refusal of the launcher raises Error."""
        f16, f32 = np.float16, np.float32
        U = np.ascontiguousarray(U, f16)
        P = len(U) if prompts is None else int(prompts)
        assert U.shape[1:] == (256, 256, 32)
        w1, b1, lw, lb, w2, b2 = weights
        w1, w2 = np.ascontiguousarray(w1, f16), np.ascontiguousarray(w2, f16)
        b1, lw, lb, b2 = (np.ascontiguousarray(a, f32) for a in (b1, lw, lb, b2))
        assert w1.shape == (9, 64, 32) and w2.shape == (9, 32, 64) and b1.shape == lw.shape == lb.shape == (64,) and b2.shape == (32,)
        features = np.ascontiguousarray(features, f32)
        assert features.ndim == 4 and features.shape[1:] == (256, 256, 32)
        index = np.ascontiguousarray(feat_index, np.int32)
        hyper_hq = np.ascontiguousarray(hyper_hq, f32)
        logits = np.zeros((len(U), 4, 256, 256), f32) if logits_in is None else np.array(logits_in, f32, order="C")
        assert len(index) >= P and hyper_hq.size >= P * 32 and logits.size >= P * 4 * 65536 and len(U) >= P
        H = np.zeros((max(P, 0), 256, 256, 64), f16) if want_h else None
        ok = C.c_int(0)
        _check_hook(cls._h().dlimg_amd_test_hq_mask_path(
            U.ctypes.data, P, w1.ctypes.data, b1.ctypes.data, lw.ctypes.data, lb.ctypes.data, w2.ctypes.data, b2.ctypes.data,
            float(eps), features.ctypes.data, len(features), index.ctypes.data_as(C.POINTER(C.c_int)), hyper_hq.ctypes.data,
            logits.ctypes.data, cls._ptr(H), C.byref(ok)))
        return logits, H, bool(ok.value)

    @classmethod
    def test_upscale_logits(cls, keys_h, W1, b1, ln_w, ln_b, eps: float, W2, b2, hyper, store_u: bool):
        """k::upscale_logits alone (dlimg_amd_test_upscale_logits), ONE launcher call on host operands with guard bytes around
        every device buffer.  keys_h (P * 4096, 256) float16, W1 (256, 256) / W2 (128, 64) float16, b1 (256,), ln_w / ln_b (64,),
        b2 (128,), hyper (P, 4, 32).  -> (logits (P, 4, 256, 256) float32, U (P, 256, 256, 32) float16 or None without store_u,
        guard bytes intact)."""
        f16, f32 = np.float16, np.float32
        keys_h, W1, W2 = (np.ascontiguousarray(a, f16) for a in (keys_h, W1, W2))
        b1, ln_w, ln_b, b2, hyper = (np.ascontiguousarray(a, f32) for a in (b1, ln_w, ln_b, b2, hyper))
        P = len(hyper)
        assert keys_h.shape == (P * 4096, 256) and W1.shape == (256, 256) and W2.shape == (128, 64) and hyper.shape == (P, 4, 32)
        assert b1.shape == (256,) and ln_w.shape == ln_b.shape == (64,) and b2.shape == (128,)
        logits = np.zeros((P, 4, 256, 256), f32)
        U = np.zeros((P, 256, 256, 32), f16) if store_u else None
        ok = C.c_int(0)
        _check_hook(cls._h().dlimg_amd_test_upscale_logits(
            keys_h.ctypes.data, P, W1.ctypes.data, b1.ctypes.data, ln_w.ctypes.data, ln_b.ctypes.data, float(eps), W2.ctypes.data,
            b2.ctypes.data, hyper.ctypes.data, int(bool(store_u)), logits.ctypes.data, cls._ptr(U), C.byref(ok)))
        return logits, U, bool(ok.value)

    @classmethod
    def test_hq_features_finish(cls, vit, emb, b_vit, b_emb):
        """k::hq_features_finish alone (dlimg_amd_test_hq_features_finish): the two GEMM results (16384, 128) float32 and the two
        biases (32,) -> (features (256, 256, 32) float32, guard bytes intact)."""
        vit, emb, b_vit, b_emb = (np.ascontiguousarray(a, np.float32) for a in (vit, emb, b_vit, b_emb))
        assert vit.shape == emb.shape == (16384, 128) and b_vit.shape == b_emb.shape == (32,)
        out = np.zeros((256, 256, 32), np.float32)
        ok = C.c_int(0)
        _check_hook(cls._h().dlimg_amd_test_hq_features_finish(vit.ctypes.data, emb.ctypes.data, b_vit.ctypes.data, b_emb.ctypes.data,
                                                               out.ctypes.data, C.byref(ok)))
        return out, bool(ok.value)

    @classmethod
    def test_hq_branch(cls, env: "Environment", branch: str, a, batch: Optional[int] = None):
        """One branch of the SAM-HQ features as the product's encoder runs it (dlimg_amd_test_hq_branch: lane 0, the entry
        SamModel::encode calls).  branch "vit" (K = the model's embed_dim, C = 256) or "emb" (K = 256, C = 64); a (B * 4096, K)
        float16, B in 1 .. 2.  -> {"A" (B * 4096, 4 C) float32, "H" (B * 16384, C) float16, "Y" (B * 16384, 128) float32, and the
        loaded operands "w1" (4 C, K) float16, "b1" (4 C,), "ln_w", "ln_b" (C,), "w2" (128, C) float16, "b2" (128,)}.
        batch: the B the hook is given when it is not len(a) / 4096 (the refusals).  A refusal raises Error."""
        f16, f32 = np.float16, np.float32
        code = {"vit": 0, "emb": 1}.get(branch, branch)
        a = None if a is None else np.ascontiguousarray(a, f16)
        B = int(batch) if batch is not None else len(a) // 4096
        K = cls.model_geometry(env)[0] if code == 0 else 256
        Cc = 256 if code == 0 else 64
        assert a is None or (a.ndim == 2 and a.shape[1] == K and len(a) >= min(max(B, 0), 2) * 4096)
        n = min(max(B, 1), 2) * 4096
        out = {"A": np.zeros((n, 4 * Cc), f32), "H": np.zeros((n * 4, Cc), f16), "Y": np.zeros((n * 4, 128), f32),
               "w1": np.zeros((4 * Cc, K), f16), "b1": np.zeros(4 * Cc, f32), "ln_w": np.zeros(Cc, f32), "ln_b": np.zeros(Cc, f32),
               "w2": np.zeros((128, Cc), f16), "b2": np.zeros(128, f32)}
        _check_hook(cls._h().dlimg_amd_test_hq_branch(env.handle(), int(code), cls._ptr(a), B,
                                                      *(out[k].ctypes.data for k in ("A", "H", "Y", "w1", "b1", "ln_w", "ln_b", "w2", "b2"))))
        return out

    @classmethod
    def test_layernorm_rows(cls, x, w, b, eps: float, act: int = 0, want_f32: bool = True, want_f16: bool = False,
                            in_place: bool = False, misalign_x: bool = False, nonfinite: Optional[int] = None,
                            rows: Optional[int] = None, dim: Optional[int] = None):
        """k::layernorm alone (dlimg_amd_test_layernorm_rows): ONE launcher call with guard bytes around every device buffer.
        x (rows, dim) float32; want_f32 / want_f16 choose the results; in_place: the launch gets out_f32 = x; misalign_x: the
        device x lies 4 bytes behind a 16-byte boundary; nonfinite (None: not asked for): the initial value of the report's int.
        rows / dim: what the launcher is told when it is not x.shape (the refusals).
        -> (float32 result or None, float16 result or None, the report's int or None, guard bytes intact).  A refusal raises Error."""
        x, w, b = (np.ascontiguousarray(v, np.float32) for v in (x, w, b))
        r = x.shape[0] if rows is None else int(rows)
        d = x.shape[1] if dim is None else int(dim)
        assert x.size >= r * d and w.size >= max(d, 1) and b.size >= max(d, 1)
        o32 = np.zeros((r, d), np.float32) if want_f32 else None
        o16 = np.zeros((r, d), np.float16) if want_f16 else None
        flag = None if nonfinite is None else C.c_int(int(nonfinite))
        ok = C.c_int(0)
        try:
            _check_hook(cls._h().dlimg_amd_test_layernorm_rows(x.ctypes.data, w.ctypes.data, b.ctypes.data, float(eps), r, d, int(act),
                                                               int(bool(in_place)), int(bool(misalign_x)), cls._ptr(o32), cls._ptr(o16),
                                                               None if flag is None else C.byref(flag), C.byref(ok)))
        except Error as e:
            e.nonfinite = None if flag is None else int(flag.value)      # a refusal returns the int as it was found
            raise
        return o32, o16, None if flag is None else int(flag.value), bool(ok.value)

    @classmethod
    def test_elementwise(cls, op: str, a, b=None, b_mod: int = 0, want_f32: bool = False, want_f16: bool = True,
                         n: Optional[int] = None):
        """The other row kernels of kernels/elementwise.hip alone (dlimg_amd_test_elementwise), guarded as test_layernorm_rows.
        "cast_f16": a float32 (n,) -> float16.  "add_cast": a float32 (n,) + b float32 (b_mod,) or None, element i taking
        b[i % b_mod] -> float32 and / or float16.  "im2col3x3": a float16 (B, 64, 64, C) -> float16 (B * 4096, 9 * C).
        n / b_mod: what the launcher is told when it is not the arrays' sizes (the refusals).
        -> (float32 result or None, float16 result or None, guard bytes intact)."""
        code = {"cast_f16": 0, "add_cast": 1, "im2col3x3": 2}[op]
        ok = C.c_int(0)
        if code == 2:
            a = np.ascontiguousarray(a, np.float16)
            B, _, _, Cc = a.shape
            assert a.shape[1:3] == (64, 64)
            o16 = np.zeros((B * 4096, 9 * Cc), np.float16)
            _check_hook(cls._h().dlimg_amd_test_elementwise(2, None, a.ctypes.data, None, Cc, B, None, o16.ctypes.data, C.byref(ok)))
            return None, o16, bool(ok.value)
        a = np.ascontiguousarray(a, np.float32).ravel()
        count_ = a.size if n is None else int(n)
        assert a.size >= count_
        b = None if b is None else np.ascontiguousarray(b, np.float32).ravel()
        assert b is None or b.size >= b_mod
        o32 = np.zeros(count_, np.float32) if (want_f32 and code == 1) else None
        o16 = np.zeros(count_, np.float16) if (want_f16 or code == 0) else None
        _check_hook(cls._h().dlimg_amd_test_elementwise(code, a.ctypes.data, None, cls._ptr(b), int(b_mod), count_, cls._ptr(o32),
                                                        cls._ptr(o16), C.byref(ok)))
        return o32, o16, bool(ok.value)

    @classmethod
    def test_matte(cls, mask, guide, radius, eps, shortcut: bool = True, time_iters: int = 0):
        """The matte kernels alone (dlimg_amd_test_matte, lib/libdlimgedit_matte_hooks.so): mask (h, w) uint8 and guide (h, w),
        (h, w, 3) or (h, w, 4) uint8 through ONE k::mask_matte call on the default device, with guard bytes around the mask,
        the guide and the workspace.  -> (matte uint8 [h, w], guard bytes intact).  Lists of equal length for all four
        arguments: that many jobs in the one call, -> (list of mattes, guards intact, launches).  guide None reaches the
        launcher as a null guide.  shortcut False: no block is skipped for being uniform (same bytes).  time_iters > 0: a
        further element, the milliseconds of one call (the mean of time_iters repetitions between two events, each on the
        mask as given).  A refusal of the launcher raises Error."""
        many = isinstance(mask, (list, tuple))
        masks = [np.array(m, np.uint8, order="C") for m in (mask if many else [mask])]      # copies: the hook writes them
        guides = [None if g is None else np.ascontiguousarray(g, np.uint8) for g in (guide if many else [guide])]
        radii = [int(r) for r in (radius if many else [radius])]
        epss = [int(e) for e in (eps if many else [eps])]
        n = len(masks)
        assert n == len(guides) == len(radii) == len(epss) and all(m.ndim == 2 for m in masks)
        channels = []
        for m, g in zip(masks, guides):
            assert g is None or (g.shape[:2] == m.shape and (g.ndim == 2 or g.ndim == 3))
            channels.append(1 if g is None or g.ndim == 2 else g.shape[2])
        ints = lambda v: (C.c_int * n)(*v)
        mp = (C.c_void_p * n)(*[m.ctypes.data for m in masks])
        gp = (C.c_void_p * n)(*[None if g is None else g.ctypes.data for g in guides])
        ok, launches, ms = C.c_int(0), C.c_int(0), C.c_float(0.0)
        lib = matte_hooks_library()
        if lib.dlimg_amd_test_matte(mp, gp, ints([m.shape[1] for m in masks]), ints([m.shape[0] for m in masks]), ints(channels),
                                    ints(radii), ints(epss), n, int(bool(shortcut)), C.byref(ok), C.byref(launches), int(time_iters),
                                    C.byref(ms)) != 0:
            msg = lib.dlimg_init().contents.last_error()
            raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")
        out = (masks, bool(ok.value), int(launches.value)) if many else (masks[0], bool(ok.value))
        return out if time_iters <= 0 else out + (float(ms.value),)

    @classmethod
    def test_cutout(cls, coverage, guide, radius, shortcut: bool = True, time_iters: int = 0):
        """The cut-out kernels alone (dlimg_amd_test_cutout, lib/libdlimgedit_matte_hooks.so): coverage (h, w) uint8 and guide
        (h, w, 3) or (h, w, 4) uint8 through ONE k::mask_cutout call on the default device, with guard bytes around the output,
        the coverage, the guide and the workspace.  -> (rgba uint8 [h, w, 4], guard bytes intact and coverage and guide on the
        device unchanged).  Lists of equal length for all three arguments: that many jobs in the one call, -> (list of rgba, ok,
        launches).  guide None reaches the launcher as a null guide.  shortcut False: no block is copied for being covered or
        bare throughout (same bytes).  time_iters > 0: a further element, the milliseconds of one call (the mean of time_iters
        repetitions between two events).  A refusal of the launcher raises Error."""
        many = isinstance(coverage, (list, tuple))
        given_a = [np.ascontiguousarray(a, np.uint8) for a in (coverage if many else [coverage])]
        given_g = [None if g is None else np.ascontiguousarray(g, np.uint8) for g in (guide if many else [guide])]
        radii = [int(r) for r in (radius if many else [radius])]
        n = len(given_a)
        assert n == len(given_g) == len(radii) and all(a.ndim == 2 for a in given_a)
        assert all(g is None or (g.ndim == 3 and g.shape[:2] == a.shape) for a, g in zip(given_a, given_g))
        covs = [a.copy() for a in given_a]                      # copies: the hook writes back what the device holds afterwards
        guides = [None if g is None else g.copy() for g in given_g]
        outs = [np.zeros(a.shape + (4,), np.uint8) for a in covs]
        ints = lambda v: (C.c_int * n)(*v)
        ptrs = lambda arrays: (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in arrays])
        ok, launches, ms = C.c_int(0), C.c_int(0), C.c_float(0.0)
        lib = matte_hooks_library()
        if lib.dlimg_amd_test_cutout(ptrs(covs), ptrs(guides), ptrs(outs), ints([a.shape[1] for a in covs]), ints([a.shape[0] for a in covs]),
                                     ints([3 if g is None else g.shape[2] for g in guides]), ints(radii), n, int(bool(shortcut)),
                                     C.byref(ok), C.byref(launches), int(time_iters), C.byref(ms)) != 0:
            msg = lib.dlimg_init().contents.last_error()
            raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")
        same = all((a == b).all() for a, b in zip(covs, given_a)) and all((a == b).all() for a, b in zip(guides, given_g))
        out = (outs, bool(ok.value) and same, int(launches.value)) if many else (outs[0], bool(ok.value) and same)
        return out if time_iters <= 0 else out + (float(ms.value),)

    @classmethod
    def test_edge(cls, masks, params, shortcut: bool = True, time_iters: int = 0):
        """The edge kernels alone (dlimg_amd_test_edge, lib/libdlimgedit_matte_hooks.so): mask (h, w) uint8 and params (offset,
        feather, border) through ONE k::mask_edge call on the default device, with guard bytes around the mask and the
        workspace.  -> (result uint8 [h, w], guard bytes intact).  Lists of equal length for both arguments: that many jobs in
        the one call, -> (list of results, guards intact, launches).  A mask None reaches the launcher as a null mask, of the
        extent params then carries as (offset, feather, border, w, h).  shortcut False: no block is filled for being of one
        polarity (same bytes).  time_iters > 0: two further elements, the milliseconds of one call (the mean of time_iters
        repetitions between two events, each on the mask as given: a device-to-device copy of it goes back first) and the
        milliseconds of those copies alone.  A refusal of the launcher raises Error."""
        many = isinstance(masks, (list, tuple))
        given = [None if m is None else np.array(m, np.uint8, order="C") for m in (masks if many else [masks])]     # copies: the hook writes them
        pars = [tuple(int(v) for v in p) for p in (params if many else [params])]
        n = len(given)
        assert n == len(pars) and all(m is None or m.ndim == 2 for m in given)
        assert all(len(p) == (3 if m is not None else 5) for m, p in zip(given, pars))
        ints = lambda v: (C.c_int * n)(*v)
        mp = (C.c_void_p * n)(*[None if m is None else m.ctypes.data for m in given])
        ok, launches, ms = C.c_int(0), C.c_int(0), (C.c_float * 2)(0.0, 0.0)
        lib = matte_hooks_library()
        if lib.dlimg_amd_test_edge(mp, ints([p[3] if m is None else m.shape[1] for m, p in zip(given, pars)]),
                                   ints([p[4] if m is None else m.shape[0] for m, p in zip(given, pars)]), ints([p[0] for p in pars]),
                                   ints([p[1] for p in pars]), ints([p[2] for p in pars]), n, int(bool(shortcut)), C.byref(ok),
                                   C.byref(launches), int(time_iters), ms) != 0:
            msg = lib.dlimg_init().contents.last_error()
            raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")
        out = (given, bool(ok.value), int(launches.value)) if many else (given[0], bool(ok.value))
        return out if time_iters <= 0 else out + (float(ms[0]), float(ms[1]))

    @classmethod
    def test_stroke_derive(cls, stroke_map: np.ndarray, pre_w: int, pre_h: int, clicks: int = STROKE_DEFAULT_CLICKS, time_iters: int = 0):
        """The stroke derivation alone (dlimg_amd_test_stroke_derive, lib/libdlimgedit_matte_hooks.so): stroke_map (h, w) uint8, of
        an image that was encoded at pre_w x pre_h, through the two launches of k::stroke_derive on the default device, with guard
        bytes around the map, the ballots and the record.  -> (record int32 [20] = ON cells, clicks, x0, y0 .. x7, y7, 0, 0 in
        cells; ballots uint64 [256, 4]; guard bytes intact); with time_iters > 0 a fourth element, the milliseconds of one
        derivation (both launches; the mean of time_iters repetitions between two events).  A refusal of the launcher raises
        Error."""
        stroke_map = np.ascontiguousarray(stroke_map, np.uint8)
        assert stroke_map.ndim == 2
        h, w = stroke_map.shape
        record, bits = np.zeros(20, np.int32), np.zeros((256, 4), np.uint64)
        ok, ms = C.c_int(0), C.c_float(0.0)
        lib = matte_hooks_library()
        if lib.dlimg_amd_test_stroke_derive(stroke_map.ctypes.data, w, h, int(pre_w), int(pre_h), int(clicks),
                                            record.ctypes.data_as(C.POINTER(C.c_int32)), bits.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            C.byref(ok), int(time_iters), C.byref(ms)) != 0:
            msg = lib.dlimg_init().contents.last_error()
            raise Error(msg.decode("utf-8", "replace") if msg else "Unknown error")
        return (record, bits, bool(ok.value)) if time_iters <= 0 else (record, bits, bool(ok.value), float(ms.value))

    NECK_GUARD = 256          # bytes of guard pattern on either side of a buffer test_neck_conv_ln allocates for one image
    NECK_GUARD_BYTE = 0xA5

    @classmethod
    def test_neck_conv_ln(cls, env: Environment, x, w, gamma, beta, eps: float, want_f16: bool = True, want_f32: bool = True,
                          own_buffer=None):
        """One launch of the encoder neck on device buffers (dlimg_amd_test_neck_conv1x1_ln / _conv3x3_ln): convolution +
        LayerNorm2d.  x: f16 [B*4096][K] with w [256][K] (1x1), or f16 [B][64][64][256] with w [256][2304] (3x3, zero pad 1,
        columns (ky*3+kx)*256 + c).  own_buffer (optional, one bool per image): image i's fp32 result goes to a device buffer
        of its own with NECK_GUARD bytes of NECK_GUARD_BYTE on either side, the others to the shared workspace.
        Returns (f16 [B*4096][256] or None, fp32 [B*4096][256] or None, flag, guards) -- guards: per image with a buffer of
        its own the (front, back) guard bytes as they are after the launch, else None."""
        x = np.ascontiguousarray(x, dtype=np.float16)
        w = np.ascontiguousarray(w, dtype=np.float16)
        gamma = np.ascontiguousarray(gamma, dtype=np.float32)
        beta = np.ascontiguousarray(beta, dtype=np.float32)
        conv3 = x.ndim == 4
        B = x.shape[0] if conv3 else x.shape[0] // 4096
        K = 2304 if conv3 else x.shape[1]
        assert x.size == B * 4096 * (256 if conv3 else K) and w.shape == (256, K) and gamma.shape == beta.shape == (256,)
        own = [False] * B if own_buffer is None else [bool(o) for o in own_buffer]
        assert len(own) == B and (want_f32 or not any(own))
        img_bytes, G = 4096 * 256 * 4, cls.NECK_GUARD
        held = []

        def dev(a=None, nbytes=0):
            ptr = cls.device_alloc(env, a.nbytes if a is not None else nbytes)
            held.append(ptr)
            if a is not None:
                cls.copy_to_device(env, ptr, a)
            return ptr

        try:
            d_x, d_w, d_g, d_b = dev(x), dev(w), dev(gamma), dev(beta)
            d_h = dev(nbytes=B * 4096 * 256 * 2) if want_f16 else None
            d_ws = dev(nbytes=B * img_bytes) if want_f32 else None
            ptrs = (C.c_void_p * B)()
            fill = np.full(img_bytes + 2 * G, cls.NECK_GUARD_BYTE, np.uint8)
            for i in range(B):
                ptrs[i] = dev(fill) + G if own[i] else None
            flag = C.c_int(-1)
            h = cls._h()
            if conv3:
                rc = h.dlimg_amd_test_neck_conv3x3_ln(d_x, B, d_w, d_g, d_b, eps, d_h, ptrs if any(own) else None, d_ws, C.byref(flag))
            else:
                rc = h.dlimg_amd_test_neck_conv1x1_ln(d_x, B, K, d_w, d_g, d_b, eps, d_h, ptrs if any(own) else None, d_ws,
                                                      C.byref(flag))
            _check_hook(rc)
            out16 = out32 = None
            guards = [None] * B
            if want_f16:
                out16 = np.empty((B * 4096, 256), np.float16)
                cls.copy_to_host(env, out16, d_h)
            if want_f32:
                out32 = np.empty((B * 4096, 256), np.float32)
                cls.copy_to_host(env, out32, d_ws)
                for i in range(B):
                    if own[i]:
                        whole = np.empty(img_bytes + 2 * G, np.uint8)
                        cls.copy_to_host(env, whole, ptrs[i] - G)
                        guards[i] = (whole[:G].copy(), whole[-G:].copy())
                        out32[i * 4096:(i + 1) * 4096] = whole[G:-G].view(np.float32).reshape(4096, 256)
            return out16, out32, flag.value, guards
        finally:
            for ptr in held:
                cls.device_free(env, ptr)

    @classmethod
    def test_attention(cls, is_global: bool, qkv, qkv_bias, rel_h, rel_w, batch: int, heads: int, hd: int):
        qkv = np.ascontiguousarray(qkv, dtype=np.float16)
        rel_h = np.ascontiguousarray(rel_h, dtype=np.float32)
        rel_w = np.ascontiguousarray(rel_w, dtype=np.float32)
        qkv_bias = None if qkv_bias is None else np.ascontiguousarray(qkv_bias, dtype=np.float32)
        out = np.empty((batch * 4096, heads * hd), dtype=np.float16)
        _check_hook(cls._h().dlimg_amd_test_attention(int(is_global), qkv.ctypes.data, cls._ptr(qkv_bias), rel_h.ctypes.data,
                                                 rel_w.ctypes.data, batch, heads, hd, out.ctypes.data))
        return out

    @classmethod
    def test_decode(cls, env: Environment, embeddings: np.ndarray, emb_index, coords, labels):
        """The product's decoder (one SamModel::decode call for all prompts) on given embeddings [n][4096][256]: prompt i
        decodes embeddings[emb_index[i]] with the packed prompt coords[i] ([2][2], resized-image pixels) and labels[i]
        ([2]).  Returns (logits [count][4][256][256], iou [count][4])."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, 4096, 256)
        idx = np.ascontiguousarray(emb_index, dtype=np.int32).reshape(-1)
        count = idx.size
        c = np.ascontiguousarray(coords, dtype=np.float32).reshape(count, 4)
        l = np.ascontiguousarray(labels, dtype=np.float32).reshape(count, 2)
        logits = np.empty((count, 4, 256, 256), dtype=np.float32)
        iou = np.empty((count, 4), dtype=np.float32)
        _check_hook(cls._h().dlimg_amd_test_decode(env.handle(), emb.shape[0], emb.ctypes.data, count, idx.ctypes.data,
                                                   c.ctypes.data, l.ctypes.data, logits.ctypes.data, iou.ctypes.data))
        return logits, iou

    @classmethod
    def test_decode_prompts(cls, env: Environment, embeddings: np.ndarray, emb_index, coords, labels, mask_planes=None,
                            mask_iou=None, want_state: bool = False):
        """The whole of SamModel::decode (one call for all prompts) on given embeddings [n][4096][256]: prompt i decodes
        embeddings[emb_index[i]] with coords[i] ([points][2], resized-image pixels) and labels[i] ([points]), 2 .. 10 points,
        the same number for every prompt.  mask_planes [count][4][256][256]: every prompt's mask input; mask_iou [count][4]:
        the predictions its plane is chosen by on the device (None: plane 0).  Returns (logits [count][4][256][256], iou
        [count][4]) and, with want_state (one prompt), {name: array} of the token-side workspaces, "mask_h" after a masked
        call."""
        emb = np.ascontiguousarray(embeddings, dtype=np.float32).reshape(-1, 4096, 256)
        idx = np.ascontiguousarray(emb_index, dtype=np.int32).reshape(-1)
        count = idx.size
        l = np.ascontiguousarray(labels, dtype=np.float32).reshape(count, -1)
        points = l.shape[1]
        c = np.ascontiguousarray(coords, dtype=np.float32).reshape(count, points, 2)
        planes = None if mask_planes is None else np.ascontiguousarray(mask_planes, dtype=np.float32).reshape(count, 4, 256, 256)
        iou4 = None if mask_iou is None else np.ascontiguousarray(mask_iou, dtype=np.float32).reshape(count, 4)
        logits = np.empty((count, 4, 256, 256), dtype=np.float32)
        iou = np.empty((count, 4), dtype=np.float32)
        state = np.empty(1 << 18, dtype=np.float32) if want_state else None      # 15 rows and mask_h need 131 k floats
        layout = C.create_string_buffer(1024)
        _check_hook(cls._h().dlimg_amd_test_decode_prompts(
            env.handle(), emb.shape[0], emb.ctypes.data, count, idx.ctypes.data, points, c.ctypes.data, l.ctypes.data,
            cls._ptr(planes), cls._ptr(iou4), logits.ctypes.data, iou.ctypes.data, cls._ptr(state),
            0 if state is None else state.size, layout, 1024))
        if not want_state:
            return logits, iou
        res, off = {}, 0
        for n, cnt in ((n, int(cnt)) for n, cnt in (item.split(":") for item in layout.value.decode().strip(",").split(","))):
            res[n] = state[off:off + cnt].copy()
            off += cnt
        return logits, iou, res

    @staticmethod
    def _named_parts(layout: bytes, flat: np.ndarray) -> dict:
        res, off = {}, 0
        for n, cnt in ((n, int(cnt)) for n, cnt in (item.split(":") for item in layout.decode().strip(",").split(","))):
            res[n] = flat[off:off + cnt].copy()
            off += cnt
        return res

    @classmethod
    def test_encoder_state(cls, env: Environment, images, image: int = 0, layer: Optional[int] = None):
        """The product's encoder (upload + one SamModel::encode on lane 0) on `images` (1 to 4 RGBA uint8 arrays or ImageViews
        whose longest side is 1024) and what it left for image `image` of that pass, {name: float32 array}: patches, stream_hi,
        stream_lo, stats ([groups][4096][2] flat), qkv and hidden of the last block, embedding, groups, split, nonfinite.
        layer (None: not asked for): additionally the loader's device operands of that block (-1: patch embed, pos_embed and
        neck) as a second dict; images may then be empty, and the first result is None."""
        views = [v if isinstance(v, ImageView) else ImageView(np.ascontiguousarray(v)) for v in images]
        D, depth, heads, mlp = cls.model_geometry(env)
        state = np.empty(4096 * (768 + 5 * D + mlp + 256 + 48) + 3, dtype=np.float32) if views else None
        operands = None
        if layer is not None:
            block = 3 * D * D + D * D + 2 * mlp * D + 12 * D + 2 * mlp + 2 * 127 * (D // heads) + 1
            other = D * 768 + D + 4096 * D + 256 * D + 256 * 2304 + 4 * 256
            operands = np.empty(other if layer < 0 else block, dtype=np.float32)
        arr = (_ImageView * max(1, len(views)))(*[v._c() for v in views])
        layout, op_layout = C.create_string_buffer(1024), C.create_string_buffer(1024)
        _check_hook(cls._h().dlimg_amd_test_encoder_state(
            env.handle(), arr, len(views), int(image), cls._ptr(state), 0 if state is None else state.size, layout, 1024,
            -2 if layer is None else int(layer), cls._ptr(operands), 0 if operands is None else operands.size, op_layout, 1024))
        taps = cls._named_parts(layout.value, state) if views else None
        return taps if layer is None else (taps, cls._named_parts(op_layout.value, operands))

    @classmethod
    def test_resize(cls, pixels: np.ndarray, channels: Channels, out_w: int, out_h: int) -> np.ndarray:
        pixels = np.ascontiguousarray(pixels)
        h, w = pixels.shape[:2]
        c = count(channels)
        out = np.empty((out_h, out_w, c), dtype=np.uint8)
        _check_hook(cls._h().dlimg_amd_test_resize(pixels.ctypes.data, w, h, w * c, int(channels), out_w, out_h,
                                              out.ctypes.data))
        return out

    @classmethod
    def birefnet_prepare_image(cls, image: np.ndarray, channels: "Channels", mean, std) -> np.ndarray:
        """BiRefNet::prepare_image: u8 [H,W,C] -> f32 [1,3,H,W] (reference: segmentation.cpp:244-256)."""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = image.shape[:2]
        mean = np.ascontiguousarray(mean, dtype=np.float32)
        std = np.ascontiguousarray(std, dtype=np.float32)
        out = np.empty((1, 3, h, w), dtype=np.float32)
        _check(cls._l().dlimg_amd_birefnet_prepare_image(image.ctypes.data, w, h, image.strides[0], int(channels),
                                                         mean.ctypes.data, std.ctypes.data, out.ctypes.data))
        return out

    @classmethod
    def birefnet_process_mask(cls, logits: np.ndarray) -> np.ndarray:
        """BiRefNet::process_mask: f32 [H,W] -> u8 [H,W] (reference: segmentation.cpp:258-270)."""
        logits = np.ascontiguousarray(logits, dtype=np.float32)
        h, w = logits.shape
        out = np.empty((h, w), dtype=np.uint8)
        _check(cls._l().dlimg_amd_birefnet_process_mask(logits.ctypes.data, w, h, out.ctypes.data))
        return out

    @classmethod
    def resize_mask(cls, mask: np.ndarray, out_w: int, out_h: int) -> np.ndarray:
        """dlimg::resize_mask: u8 [H,W] -> u8 [out_h,out_w], box filter (reference: image.cpp:53-62)."""
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w = mask.shape
        out = np.empty((out_h, out_w), dtype=np.uint8)
        _check(cls._l().dlimg_amd_resize_mask(mask.ctypes.data, w, h, mask.strides[0], out_w, out_h, out.ctypes.data))
        return out

    @classmethod
    def bench_prepost(cls, batch: int = 16, iters: int = 50, working_set_mb: int = 768) -> Tuple[float, float]:
        """(ms per launch of the pre-processing kernel, of the post-processing kernel) on `batch` images / masks; launches
        rotate over `working_set_mb` MB of distinct inputs and outputs (nothing Infinity-Cache resident)."""
        pre, post = C.c_double(), C.c_double()
        _check_hook(cls._h().dlimg_amd_bench_prepost(batch, iters, working_set_mb, C.byref(pre), C.byref(post)))
        return pre.value, post.value

    @classmethod
    def bench_attention(cls, is_global: bool, heads: int = 12, hd: int = 64, batch: int = 1, iters: int = 50) -> float:
        """ms per launch of the encoder attention kernel alone, device-resident random data."""
        ms = C.c_double()
        _check_hook(cls._h().dlimg_amd_bench_attention(int(is_global), batch, heads, hd, iters, C.byref(ms)))
        return ms.value

    @classmethod
    def bench_gemm(cls, M: int, N: int, K: int, act: int = 0, iters: int = 20, flavour: int = 0, tile: int = -1,
                   shared: bool = False, streams: int = 1) -> float:
        ms = C.c_double()
        _check_hook(cls._h().dlimg_amd_bench_gemm_streams(M, N, K, act, flavour, tile, int(shared), streams, iters,
                                                     C.byref(ms)))
        return ms.value

    @classmethod
    def bench_gemm_stamps(cls, M: int, N: int, K: int, act: int = 0, iters: int = 20, flavour: int = 0, tile: int = 9,
                          streams: int = 1, groups: int = 4096):
        """(ms per GEMM, stamps [groups][4] u64: main-loop cycles, main-loop 100 MHz ticks, kernel cycles, kernel ticks)."""
        ms = C.c_double()
        st = np.zeros((groups, 4), np.uint64)
        _check_hook(cls._h().dlimg_amd_bench_gemm_stamps(M, N, K, act, flavour, tile, 0, streams, iters, C.byref(ms),
                                                    st.ctypes.data, groups))
        return ms.value, st
