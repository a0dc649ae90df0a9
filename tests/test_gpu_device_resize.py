"""Images of any size on the asynchronous device-resident path (dlimg_amd_encode_and_mask / dlimg_amd_encode_only).

The library resamples an image whose longest side is not 1024 with one fused kernel pair (csrc/kernels/resize.hip, K18:
rows -> fp32 planes, columns + sRGB encode + pre-processing -> the f16 patch matrix) for all images of a pass at once;
slots 3 / 13 upload a host image and run the same launch.

  exactness   the embedding of an image passed at its own size (resampled on the device) is BIT-EQUAL to the embedding of
              the same image resampled on the CPU by oracle/stb_resize.py and passed at the encoder's size (never resampled
              on the device) -- every size at which the kernels take another path, every channel order, a padded stride
  device path the masks of views in device memory equal slot 3 + slot 4 on the host copy, byte for byte and width x height
              long: requests of one size, four sizes coalesced into one pass, a batch call, a pass that mixes a 1024 image
              with others, and encode_only
  steady state two sizes alternating for 20 requests, and more sizes than a lane's table cache holds
"""
import numpy as np
import pytest

from conftest import halton_points

# (w, h) -> the extent the library encodes it at (longest side to 1024: int(side * scale + 0.5) in fp32)
SIZES = {
    (1600, 1200): (1024, 768),      # down-sampling, landscape
    (640, 480): (1024, 768),        # up-sampling
    (600, 1500): (410, 1024),       # portrait
    (1031, 517): (1024, 513),       # odd sizes; taps that clamp at both edges
    (2048, 16): (1024, 8),          # a result only 8 rows high
    (33, 1025): (33, 1024),         # a one-pixel reduction on the long side
    # 39 x smaller: the source bytes of 256 neighbouring outputs (40 KB of RGBA) exceed the 32 KB the row stage keeps in
    # LDS, so it reads its taps from memory instead -- the only other path of the kernel pair
    (40000, 40): (1024, 1),
}
ODD = (1031, 517)


def pattern_image(seed: int, w: int, h: int, c: int = 4) -> np.ndarray:
    """A cheap image with structure at every scale: two crossed gradients, a checker of 37-pixel cells and noise."""
    rng = np.random.default_rng(5000 + seed)
    x = np.arange(w, dtype=np.float32)[None, :]
    y = np.arange(h, dtype=np.float32)[:, None]
    img = np.zeros((h, w, c), np.uint8)
    for k in range(c):
        f = 40.0 + 170.0 * ((x * (k + 1) / w + y * (c - k) / h) % 1.0) + 35.0 * (((x // 37) + (y // 37) + k) % 2)
        img[:, :, k] = np.clip(f + rng.uniform(-12, 12, (h, w)), 0, 255).astype(np.uint8)
    return img


def strided(img: np.ndarray, extra: int):
    """The same pixels in rows of w * C + extra bytes (the padding filled with 0xAB): (array view [h, w, C], stride)."""
    h, w, c = img.shape
    stride = w * c + extra
    buf = np.full((h, stride), 0xAB, np.uint8)
    buf[:, :w * c] = img.reshape(h, w * c)
    return np.lib.stride_tricks.as_strided(buf, (h, w, c), (stride, c, 1)), stride


def test_sizes_resize_to_what_the_library_computes():
    """CPU, oracle alone: every size of the table is encoded at the extent written next to it, longest side 1024."""
    from oracle import sam_oracle as O
    from oracle.stb_resize import resize_srgb
    f32 = np.float32
    for (w, h), want in SIZES.items():
        scale = f32(1024) / f32(max(w, h))
        mine = (int(f32(f32(w) * scale) + f32(0.5)), int(f32(f32(h) * scale) + f32(0.5)))
        assert mine == want and O.ResizeLongestSide().target_extent(w, h) == want, (w, h, mine)
        assert max(want) == 1024 and min(want) >= 1
    for (w, h) in [(2048, 16), (33, 1025)]:                  # ... and the oracle's resampler produces that extent
        rw, rh = SIZES[(w, h)]
        assert resize_srgb(pattern_image(0, w, h), rw, rh).shape == (rh, rw, 4)


@pytest.fixture(scope="module")
def setup(model_dirs):
    from dlimgedit_amd import api
    mdir, _, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    return api, env


def channel_cases(api):
    C = api.Channels
    return {"rgba": (C.rgba, 4, 0), "rgb": (C.rgb, 3, 0), "bgra": (C.bgra, 4, 0), "argb": (C.argb, 4, 0), "mask": (C.mask, 1, 0),
            "rgba_stride12": (C.rgba, 4, 12),       # stride = w * C + 12
            "rgba_stride13": (C.rgba, 4, 13),       # rows that start off a 4-byte boundary: no whole-pixel LDS reads
            "rgb_stride12": (C.rgb, 3, 12)}


EXACT_CASES = [(w, h, "rgba") for (w, h) in SIZES] + \
              [(ODD[0], ODD[1], v) for v in ("rgb", "bgra", "argb", "mask", "rgba_stride12", "rgba_stride13", "rgb_stride12")]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,variant", EXACT_CASES, ids=[f"{w}x{h}-{v}" for w, h, v in EXACT_CASES])
def test_device_resize_is_bit_exact(setup, w, h, variant):
    """Path A: the image at its own size through slot 3 (resampled by the fused kernels).  Path B: the image resampled on
    the CPU by the oracle to the same extent, through slot 3 (no device resize at all).  The embeddings are bit-equal."""
    from oracle.stb_resize import resize_srgb
    api, env = setup
    channels, c, extra = channel_cases(api)[variant]
    rw, rh = SIZES[(w, h)]
    img = pattern_image(w + h, w, h, c)
    if extra:
        arr, stride = strided(img, extra)
        view = api.ImageView(arr, channels, stride)
    else:
        view = api.ImageView(img, channels)
    seg = api.Segmentation.process(view, env)
    got = api.ext.get_embedding(seg)
    seg.close()
    small = resize_srgb(img, rw, rh)
    assert small.shape == (rh, rw, c)
    seg = api.Segmentation.process(api.ImageView(small, channels), env)
    want = api.ext.get_embedding(seg)
    seg.close()
    assert np.isfinite(want).all() and np.array_equal(got, want), \
        f"{np.count_nonzero(got != want)} of {want.size} embedding values differ, max {np.abs(got - want).max()}"


# ---- the device path ------------------------------------------------------------------------------------------------

class DeviceImages:
    """Images in device memory with one mask buffer per request; frees what it allocated."""

    def __init__(self, api, env):
        self.api, self.env, self.ext = api, env, api.ext
        self.owned = []

    def put(self, array: np.ndarray) -> int:
        p = self.ext.device_alloc(self.env, array.nbytes)
        self.owned.append(p)
        self.ext.copy_to_device(self.env, p, array)
        return p

    def mask(self, w: int, h: int) -> int:
        p = self.ext.device_alloc(self.env, w * h)
        self.owned.append(p)
        self.ext.copy_to_device(self.env, p, np.full(w * h, 0x5A, np.uint8))     # neither 0 nor 255: every byte must be written
        return p

    def fetch(self, ptr: int, w: int, h: int) -> np.ndarray:
        out = np.empty((h, w), np.uint8)
        self.ext.copy_to_host(self.env, out, ptr)
        return out

    def close(self):
        for p in self.owned:
            self.ext.device_free(self.env, p)
        self.owned = []


@pytest.fixture
def dev(setup):
    api, env = setup
    d = DeviceImages(api, env)
    yield d
    api.ext.synchronize(env)
    d.close()


_host = {}


def host_reference(api, env, w, h):
    """(image, its three Halton points, the masks of slot 3 + slot 4 on the host copy); computed once per size."""
    if (w, h) not in _host:
        img = pattern_image(w * 3 + h, w, h, 4)
        pts = [api.Point(x, y) for x, y in halton_points(3, w, h)]
        seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
        masks = [seg.compute_mask(p) for p in pts]
        seg.close()
        for m in masks:
            assert m.shape == (h, w) and m.dtype == np.uint8
            m.setflags(write=False)
        img.setflags(write=False)
        _host[(w, h)] = (img, pts, masks)
    return _host[(w, h)]


DEVICE_SIZES = [s for s in SIZES if s != (40000, 40)] + [(40000, 40)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", DEVICE_SIZES, ids=[f"{w}x{h}" for w, h in DEVICE_SIZES])
def test_device_resident_masks_equal_the_host_path(setup, dev, w, h):
    """Three point prompts on one image in device memory, queued before the synchronise: each mask is width x height bytes
    and byte-equal to slot 3 + slot 4 on the host copy.  (Byte-equal masks do not see a one-LSB error of a resampled
    pixel; test_device_resize_is_bit_exact proves the kernels bit for bit, this test that device memory reaches them.)"""
    api, env = setup
    img, pts, want = host_reference(api, env, w, h)
    src = dev.put(img)
    masks = [dev.mask(w, h) for _ in pts]
    for p, m in zip(pts, masks):
        api.ext.encode_and_mask(env, api.ext.device_views([src], w, h), [p], [m])
    api.ext.synchronize(env)
    for m, ref in zip(masks, want):
        assert np.array_equal(dev.fetch(m, w, h), ref)


def run_requests(api, env, dev, sizes, one_call: bool):
    """One request per size (first Halton point), as separate calls or as one call; returns the (got, want) mask pairs."""
    srcs, masks, pts, want = [], [], [], []
    for (w, h) in sizes:
        img, p, ref = host_reference(api, env, w, h)
        srcs.append(dev.put(img))
        masks.append(dev.mask(w, h))
        pts.append(p[0])
        want.append(ref[0])
    ws, hs = [s[0] for s in sizes], [s[1] for s in sizes]
    if one_call:
        api.ext.encode_and_mask(env, api.ext.device_views(srcs, ws, hs), pts, masks)
    else:
        for i in range(len(sizes)):
            api.ext.encode_and_mask(env, api.ext.device_views([srcs[i]], ws[i], hs[i]), [pts[i]], [masks[i]])
    api.ext.synchronize(env)
    return [(dev.fetch(m, w, h), ref) for m, (w, h), ref in zip(masks, sizes, want)]


@pytest.mark.gpu
def test_four_sizes_coalesce_into_one_pass(setup, dev):
    """Four single requests of four different sizes, queued before the synchronise, share one pass of four images."""
    api, env = setup
    before = api.ext.queue_config(env)
    assert before["coalesce"] == 4
    sizes = [(1600, 1200), (640, 480), (600, 1500), (1031, 517)]
    for w, h in sizes:
        host_reference(api, env, w, h)                       # (the host path's own one-image passes happen here)
    before = api.ext.queue_config(env)
    for got, want in run_requests(api, env, dev, sizes, one_call=False):
        assert np.array_equal(got, want)
    after = api.ext.queue_config(env)
    assert after["one_image_passes"] == before["one_image_passes"]      # none of the four ran on its own


@pytest.mark.gpu
def test_batch_call_of_mixed_sizes(setup, dev):
    """One call with more views than the queue is wide runs as one pass: five sizes, one of them at 1024 already."""
    api, env = setup
    sizes = [(2048, 16), (1024, 700), (33, 1025), (640, 480), (1031, 517)]
    assert len(sizes) >= api.ext.queue_config(env)["coalesce"]
    for got, want in run_requests(api, env, dev, sizes, one_call=True):
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_a_1024_image_and_another_share_a_pass(setup, dev):
    """Four queued requests, 1024-sized and not, alternating: the pass takes the pre-processing launch for the former and the
    fused resize for the latter; neither disturbs the other's slot."""
    api, env = setup
    sizes = [(1024, 700), (600, 1500), (700, 1024), (640, 480)]
    for got, want in run_requests(api, env, dev, sizes, one_call=False):
        assert np.array_equal(got, want)


@pytest.mark.gpu
def test_encode_only_takes_any_size(setup, dev):
    api, env = setup
    w, h = ODD
    img, _, _ = host_reference(api, env, w, h)
    src = dev.put(img)
    api.ext.encode_only(env, api.ext.device_views([src], w, h))          # raises unless the call returns 0
    api.ext.encode_only(env, api.ext.device_views([src, src], w, h))
    api.ext.synchronize(env)


@pytest.mark.gpu
def test_a_view_too_narrow_to_encode_is_refused_when_it_is_queued(setup, dev):
    """4000 x 1 would be encoded at 1024 x 0: refused by the call itself, nothing is left for synchronize to report."""
    api, env = setup
    src = dev.put(np.zeros((1, 4000, 4), np.uint8))
    with pytest.raises(api.Error, match="too narrow"):
        api.ext.encode_and_mask(env, api.ext.device_views([src], 4000, 1), [api.Point(5, 0)], [dev.mask(4000, 1)])
    api.ext.synchronize(env)


# ---- steady state ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_two_sizes_alternating_stay_coalesced(setup, dev):
    """20 requests, two sizes in turn: five passes of four; requests 3-20 give the masks of requests 1-2, which are those of
    the host path, and no request ran in a pass of its own."""
    api, env = setup
    sizes = [(320, 240), (200, 300)]
    ref = [host_reference(api, env, w, h) for w, h in sizes]
    srcs = [dev.put(r[0]) for r in ref]
    masks = [dev.mask(*sizes[i % 2]) for i in range(20)]
    before = api.ext.queue_config(env)
    for i in range(20):
        w, h = sizes[i % 2]
        api.ext.encode_and_mask(env, api.ext.device_views([srcs[i % 2]], w, h), [ref[i % 2][1][0]], [masks[i]])
    api.ext.synchronize(env)
    after = api.ext.queue_config(env)
    assert after["coalesce"] == before["coalesce"] >= 2
    assert after["one_image_passes"] == before["one_image_passes"]
    got = [dev.fetch(masks[i], *sizes[i % 2]) for i in range(20)]
    for i in range(2):
        assert np.array_equal(got[i], ref[i][2][0])
    for i in range(2, 20):
        assert np.array_equal(got[i], got[i % 2]), i


@pytest.mark.gpu
def test_more_sizes_than_the_table_cache_holds(model_dirs, monkeypatch):
    """A lane remembers the contributor tables of 64 (in, out) axis pairs.  36 images of 72 distinct pairs through an
    environment of ONE lane, then the first eight sizes again (their tables evicted in between): every mask equals the host
    path's on the same environment."""
    from dlimgedit_amd import api
    monkeypatch.setenv("DLIMGEDIT_LANES", "1")
    mdir, _, _ = model_dirs("vit_test")
    env = api.Environment(api.Options(api.Backend.gpu, mdir))
    assert api.ext.lane_count(env) == 1
    dev = DeviceImages(api, env)
    try:
        sizes = [(100 + i, 60 + i) for i in range(36)]
        from oracle import sam_oracle as O
        pairs = set()
        for w, h in sizes:
            rw, rh = O.ResizeLongestSide().target_extent(w, h)
            pairs |= {(w, rw), (h, rh)}
        assert len(pairs) == 72 > 64
        imgs = [pattern_image(i, w, h) for i, (w, h) in enumerate(sizes)]
        pts = [api.Point(w // 3, h // 2) for w, h in sizes]
        want = []
        for im, p in zip(imgs, pts):
            seg = api.Segmentation.process(api.ImageView(im, api.Channels.rgba), env)
            want.append(seg.compute_mask(p))
            seg.close()
        srcs = [dev.put(im) for im in imgs]
        order = list(range(36)) + list(range(8))
        masks = [dev.mask(*sizes[i]) for i in order]
        for at in range(0, len(order), 4):                    # passes of four, each a batch call
            ids = order[at:at + 4]
            views = api.ext.device_views([srcs[i] for i in ids], [sizes[i][0] for i in ids], [sizes[i][1] for i in ids])
            api.ext.encode_and_mask(env, views, [pts[i] for i in ids], masks[at:at + 4])
        api.ext.synchronize(env)
        for k, i in enumerate(order):
            assert np.array_equal(dev.fetch(masks[k], *sizes[i]), want[i]), (k, sizes[i])
    finally:
        api.ext.synchronize(env)
        dev.close()
        env.close()

