"""Measurements of the stroke mark (clicks sampled from a caller's scribble on the GPU), ViT-B synthetic weights.

    python tools/stroke_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::stroke_derive alone (both launches; dlimg_amd_test_stroke_derive of lib/libdlimgedit_matte_hooks.so) at 1024 x 1024,
           1800 x 1200, 4000 x 3000 and 4096 x 4096: microseconds per derivation of 3 and of 8 clicks, for a thin scribble (few
           ON cells) and for a full map (65536 ON cells: the longest sampling rounds) -- and, next to it, k::lasso_derive on the
           same full map (dlimg_amd_test_lasso_derive), whose two launches do not read the image
  query    a scribble-only call (a foreground and a background stroke, 3 clicks each) against the SAME prompt sent as explicit
           clicks at tests/stroke_ref.py's pixels, on one image of each extent: wall clock of the calling thread (median and
           minimum of the repetitions after a warm-up)

Kernel times are means between two events on the null stream; the maps are numpy arrays of the caller's (the staging road).
"""
import argparse
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STEPS = {"kernel": 180, "query": 400}       # seconds
EXTENTS = [(1024, 1024), (1800, 1200), (4000, 3000), (4096, 4096)]


def _scribble(w, h, at=0.4):
    import numpy as np
    m = np.zeros((h, w), np.uint8)
    t = np.arange(int(0.6 * w))
    x = int(0.2 * w) + t
    y = (at * h + 0.1 * h * np.sin(t * 6.0 / len(t))).astype(np.int64)
    for d in (-1, 0, 1):
        m[y + d, x] = 255
    return m


def step_kernel():
    import numpy as np
    import stroke_ref
    from dlimgedit_amd import api
    for w, h in EXTENTS:
        pre_w, pre_h = stroke_ref.pre_extent(w, h)
        for name, m in (("scribble", _scribble(w, h)), ("full", np.full((h, w), 255, np.uint8))):
            for clicks in (3, 8):
                api.ext.test_stroke_derive(m, pre_w, pre_h, clicks, time_iters=20)          # warm-up
                rec, _, ok, ms = api.ext.test_stroke_derive(m, pre_w, pre_h, clicks, time_iters=200)
                print(f"kernel {w}x{h} {name} {clicks} clicks: {ms * 1e3:.2f} us per derivation (2 launches, {w * h / ms / 1e9:.2f} TB/s of "
                      f"map), record {rec.tolist()[:2 + 2 * clicks]}; guards intact {ok}")
        full = np.full((h, w), 255, np.uint8)
        api.ext.test_lasso_derive(full, pre_w, pre_h, time_iters=20)
        _, ok, ms = api.ext.test_lasso_derive(full, pre_w, pre_h, time_iters=200)
        print(f"kernel {w}x{h} full, k::lasso_derive for comparison: {ms * 1e3:.2f} us per derivation (2 launches, the plane given)")


def step_query():
    import numpy as np
    import stroke_ref
    from dlimgedit_amd import api, weights as W
    from dlimgedit_amd.sam_config import get_config
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        W.write_synthetic_model_dir(d, get_config("vit_b"), seed=7, mask_branch=True)
        env = api.Environment(api.Options(api.Backend.gpu, d))
        for w, h in EXTENTS[:3]:
            img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
            fg, bg, out = _scribble(w, h), _scribble(w, h, 0.8), api._mask_image(seg.extent())
            pixels = stroke_ref.derive(fg, 3) + stroke_ref.derive(bg, 3)
            clicks = [api.Point(x, y) for x, y in pixels]
            calls = [("explicit (6 clicks)", lambda: seg.compute_mask_clicks(clicks, [1, 1, 1, 0, 0, 0], out=out)),
                     ("stroke marks", lambda: seg.scribble(fg, bg, out=out))]
            masks = []
            for name, call in calls:
                for _ in range(5):
                    call()
                masks.append(out.copy())
                times = []
                for _ in range(40):
                    t0 = time.perf_counter()
                    call()
                    times.append((time.perf_counter() - t0) * 1e3)
                print(f"query {w}x{h} {name}: wall median {statistics.median(times):.3f} ms, min {min(times):.3f} ms")
            print(f"query {w}x{h}: the two masks are byte-equal: {bool((masks[0] == masks[1]).all())}")
            seg.close()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        step_kernel() if args.step == "kernel" else step_query()
        return 0
    lines = []
    for step, limit in STEPS.items():
        try:
            r = subprocess.run([sys.executable, __file__, "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            lines.append(f"{step}: no result within {limit} s; nothing more is started")
            break
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines.append(f"{step}: exit status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        Path(args.out).write_text(text)
    return 0 if all("nothing more is started" not in l for l in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
