"""Measurements of the edge mark (grow, shrink, feather and border a mask, on the GPU), ViT-B synthetic weights.

    python tools/edge_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::mask_edge alone (dlimg_amd_test_edge of lib/libdlimgedit_matte_hooks.so) at 4000 x 3000 for R = 3, 17 and 129 --
           (2, 0, 0), (8, 4, 4) and (64, 32, 32) -- on a disc (a real-looking mask: most blocks are of one polarity) and on 31-pixel
           blobs (edges everywhere), with the shortcut and without it: milliseconds per call, the mean between two events, less the
           device-to-device copy that puts the mask back in front of every call; the bytes of the disc are compared with
           tests/edge_ref.py once per R.  Beside each time two yardsticks of the same run: the time the kernels' own 14 bytes per
           pixel (mask_edge.hip) would take at the rate that copy reached (it moves 2 bytes per pixel), and k::mask_matte at radius
           16 on the same extent and the disc.
  query    one click prompt on a 4000 x 3000 image without the mark and with it ((2, 0, 0), (8, 4, 4), (64, 32, 32)), result in the
           caller's memory: wall clock of the calling thread and, with the stage clocks on, the milliseconds and launches of
           stage 7 (post) per query.
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

STEPS = {"kernel": 400, "query": 400}       # seconds
W, H = 4000, 3000
PARAMS = [(2, 0, 0), (8, 4, 4), (64, 32, 32)]        # R = 3, 17, 129
KERNEL_BYTES_PER_PIXEL = 14                           # kernels/mask_edge.hip, no block uniform, R = 129
COPY_BYTES_PER_PIXEL = 2


def step_kernel():
    import numpy as np
    import edge_ref as ER
    from test_edge_ref import blobs
    from dlimgedit_amd import api
    yy, xx = np.mgrid[0:H, 0:W]
    disc = np.where(np.hypot(xx - 0.5 * W, yy - 0.5 * H) < 0.3 * H, 255, 0).astype(np.uint8)
    noisy = blobs(W, H, np.random.default_rng(1), cell=31)
    for p in PARAMS:
        R = ER.reach(*p)
        want = ER.edge(disc, *p)
        for name, mask in (("disc", disc), ("blobs", noisy)):
            for shortcut in (True, False):
                api.ext.test_edge(mask, p, shortcut=shortcut, time_iters=3)        # warm-up
                out, ok, ms, copy_ms = api.ext.test_edge(mask, p, shortcut=shortcut, time_iters=20)
                same = "" if name != "disc" else f"; bytes equal the reference {bool((out == want).all())}"
                print(f"kernel {W}x{H} R{R} {p} {name} shortcut {int(shortcut)}: {ms - copy_ms:.3f} ms per call ({2 + int(shortcut)} launches); "
                      f"the copy {copy_ms:.3f} ms = {COPY_BYTES_PER_PIXEL * W * H / copy_ms / 1e6:.0f} GB/s, at which "
                      f"{KERNEL_BYTES_PER_PIXEL} bytes a pixel take {copy_ms * KERNEL_BYTES_PER_PIXEL / COPY_BYTES_PER_PIXEL:.3f} ms; "
                      f"guards intact {ok}{same}")
    rgba = _image(W, H)
    for shortcut in (True, False):
        api.ext.test_matte(disc, rgba, 16, 650, shortcut=shortcut, time_iters=3)
        _, ok, ms = api.ext.test_matte(disc, rgba, 16, 650, shortcut=shortcut, time_iters=20)
        print(f"kernel {W}x{H} r16 k::mask_matte disc shortcut {int(shortcut)}: {ms:.3f} ms per call (3 launches + a {W * H / 1e6:.0f} MB "
              f"copy); guards intact {ok}")


def step_query():
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
        calls = [("no mark", lambda: seg.compute_mask_clicks(click, out=out))]
        for p in PARAMS:
            calls.append((f"edge mark {p}", lambda p=p: seg.compute_mask_clicks(click, out=out, edge=p)))
        for name, call in calls:
            for _ in range(3):
                call()
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
                  f"mask {float((out >= 128).mean()):.3f} covered")
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
