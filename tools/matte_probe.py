"""Measurements of the matte mark (an image-guided soft edge for a prompt's mask, on the GPU), ViT-B synthetic weights.

    python tools/matte_probe.py [--out FILE] [--plain-only]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::mask_matte alone (three launches; dlimg_amd_test_matte of lib/libdlimgedit_matte_hooks.so) at 4000 x 3000, radius
           16, on a disc (a real-looking mask) and on a random 0 / 255 mask, with the uniform-block shortcut and without it:
           milliseconds per call, the mean between two events; every repetition starts from the mask as given, so a call
           includes a device copy of w * h bytes
  query    one click prompt on a 4000 x 3000 image with the mark (radius 16) and without it: wall clock of the calling thread
           and, with the stage clocks on, the milliseconds, launches and bytes of stage 7 (post) per query.  The delivered
           mask is whatever the synthetic model gives; its covered fraction is printed.  `--plain-only` times the call without
           the mark alone, which a build without the mark serves too.
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STEPS = {"kernel": 240, "query": 400}       # seconds
W, H, RADIUS = 4000, 3000, 16


def _image(w, h):
    import numpy as np
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 4), np.uint8)
    for c in range(3):
        img[:, :, c] = np.clip(128 + 60 * np.sin(xx * 0.01 * (c + 1)) * np.cos(yy * 0.013) + rng.uniform(-8, 8, (h, w)), 0, 255).astype(np.uint8)
    img[:, :, 3] = 255
    return img


def step_kernel():
    import numpy as np
    from dlimgedit_amd import api
    yy, xx = np.mgrid[0:H, 0:W]
    disc = np.where((xx - 0.5 * W) ** 2 + (yy - 0.5 * H) ** 2 <= (0.3 * H) ** 2, 255, 0).astype(np.uint8)
    rand = (255 * np.random.default_rng(1).integers(0, 2, (H, W))).astype(np.uint8)
    guide = _image(W, H)
    for name, mask in (("disc", disc), ("random", rand)):
        for shortcut in (True, False):
            api.ext.test_matte(mask, guide, RADIUS, 650, shortcut=shortcut, time_iters=3)        # warm-up
            out, ok, ms = api.ext.test_matte(mask, guide, RADIUS, 650, shortcut=shortcut, time_iters=20)
            soft = int(((out > 0) & (out < 255)).sum())
            print(f"kernel {W}x{H} r{RADIUS} {name} shortcut {int(shortcut)}: {ms:.3f} ms per call (3 launches + a {W * H / 1e6:.0f} MB copy), "
                  f"{soft} soft pixels; guards intact {ok}")


def step_query(plain_only=False):
    import numpy as np
    from dlimgedit_amd import api, weights as Wt
    from dlimgedit_amd.sam_config import get_config
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        Wt.write_synthetic_model_dir(d, get_config("vit_b"), seed=7)
        env = api.Environment(api.Options(api.Backend.gpu, d))
        img = _image(W, H)
        seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
        out = api._mask_image(seg.extent())
        click = [api.Point(W // 2, H // 2)]
        calls = [("without the mark", lambda: seg.compute_mask_clicks(click, out=out))]
        if not plain_only:
            calls.append((f"matte mark r{RADIUS}", lambda: seg.compute_mask_clicks(click, out=out, matte=(img, RADIUS, 0))))
        for name, call in calls:
            for _ in range(3):
                call()
            covered, soft = float((out > 0).mean()), int(((out > 0) & (out < 255)).sum())
            times = []
            for _ in range(20):
                t0 = time.perf_counter()
                call()
                times.append((time.perf_counter() - t0) * 1e3)
            api.ext.set_profiling(env, True)
            api.ext.take_stage_stats(env)
            for _ in range(10):
                call()
            st = api.ext.take_stage_stats(env)
            api.ext.set_profiling(env, False)
            print(f"query {W}x{H} {name}: wall median {statistics.median(times):.3f} ms, min {min(times):.3f} ms; per query post "
                  f"{st['post']['ms'] / 10:.4f} ms in {st['post']['launches'] / 10:g} launches, {st['post']['work'] / 10:.0f} bytes; "
                  f"{covered:.3f} covered, {soft} soft pixels")
        seg.close()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    if args.step:
        step_kernel() if args.step == "kernel" else step_query(args.plain_only)
        return 0
    lines = []
    for step, limit in STEPS.items():
        if step == "kernel" and args.plain_only:
            continue
        cmd = [sys.executable, __file__, "--step", step] + (["--plain-only"] if args.plain_only else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
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
