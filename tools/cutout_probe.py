"""Measurements of the cut-out mark (a matte's foreground colours as RGBA, on the GPU), ViT-B synthetic weights.

    python tools/cutout_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::mask_cutout alone (dlimg_amd_test_cutout of lib/libdlimgedit_matte_hooks.so) at 4000 x 3000, radius 16, guides of
           3 and 4 channels, on a soft-edged disc (a real-looking coverage) and on uniform noise (no block qualifies for the
           shortcut), with the shortcut and without it: milliseconds per call, the mean between two events; the bytes of the
           disc are compared with tests/cutout_ref.py once.  Then k::mask_matte on the same image and the disc's 0 / 255 mask, so
           that a kernel trace of this step (rocprofv3 --kernel-trace --stats -- python tools/cutout_probe.py --step kernel)
           holds matte_out_kernel, the nearest existing kernel, beside cutout_out_kernel.
  query    one click prompt on a 4000 x 3000 image with a matte mark (radius 16), and with a cut-out mark (radius 16) behind
           it, result in the caller's memory and in create_image memory: wall clock of the calling thread and, with the stage
           clocks on, the milliseconds and launches of stage 7 (post) per query.
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

from matte_probe import _image  # noqa: E402

STEPS = {"kernel": 300, "query": 400}       # seconds
W, H, RADIUS = 4000, 3000, 16


def step_kernel():
    import numpy as np
    import cutout_ref as CR
    from dlimgedit_amd import api
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.hypot(xx - 0.5 * W, yy - 0.5 * H)
    disc = np.clip(255 * (0.5 + (0.3 * H - d) / 24.0), 0, 255).astype(np.uint8)         # a band of 24 pixels
    noise = np.random.default_rng(1).integers(0, 256, (H, W)).astype(np.uint8)
    rgba = _image(W, H)
    rgb = np.ascontiguousarray(rgba[:, :, :3])
    want = CR.cutout(rgb, disc, RADIUS)
    for name, cov in (("soft disc", disc), ("noise", noise)):
        for guide in (rgb, rgba):
            for shortcut in (True, False):
                api.ext.test_cutout(cov, guide, RADIUS, shortcut=shortcut, time_iters=3)        # warm-up
                out, ok, ms = api.ext.test_cutout(cov, guide, RADIUS, shortcut=shortcut, time_iters=20)
                same = "" if name != "soft disc" else f"; bytes equal the reference {bool((out == want).all())}"
                print(f"kernel {W}x{H} r{RADIUS} {name} {guide.shape[2]} channels shortcut {int(shortcut)}: {ms:.3f} ms per call "
                      f"({1 + int(shortcut)} launches), {int(((cov > 0) & (cov < 255)).sum())} soft pixels; guards intact {ok}{same}")
    mask = np.where(disc >= 128, 255, 0).astype(np.uint8)
    for shortcut in (True, False):
        api.ext.test_matte(mask, rgba, RADIUS, 650, shortcut=shortcut, time_iters=3)
        _, ok, ms = api.ext.test_matte(mask, rgba, RADIUS, 650, shortcut=shortcut, time_iters=20)
        print(f"kernel {W}x{H} r{RADIUS} k::mask_matte disc shortcut {int(shortcut)}: {ms:.3f} ms per call (3 launches + a {W * H / 1e6:.0f} MB "
              f"copy); guards intact {ok}")


def step_query():
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
        own = np.zeros((H, W, 4), np.uint8)
        table = api.Image(api.Extent(W, H), api.Channels.rgba).pixels().reshape(H, W, 4)
        click = [api.Point(W // 2, H // 2)]
        calls = [(f"matte mark r{RADIUS}", lambda: seg.compute_mask_clicks(click, out=out, matte=(img, RADIUS, 0))),
                 (f"matte + cut-out mark r{RADIUS}, own memory", lambda: seg.compute_mask_clicks(click, out=out, matte=(img, RADIUS, 0), cutout=(RADIUS, own))),
                 (f"matte + cut-out mark r{RADIUS}, create_image memory", lambda: seg.compute_mask_clicks(click, out=out, matte=(img, RADIUS, 0), cutout=(RADIUS, table)))]
        for name, call in calls:
            for _ in range(3):
                call()
            soft = int(((out > 0) & (out < 255)).sum())
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
                  f"{soft} soft pixels")
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
