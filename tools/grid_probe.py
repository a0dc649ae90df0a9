"""Measurements of the grid prompt ("segment everything"), ViT-B synthetic weights, one 1024 x 1024 image.

    python tools/grid_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  map      milliseconds per label map at side 16 and 32, against the nearest thing the library could do without grid prompts:
           ONE batch call of side * side one-point prompts, which delivers side * side full masks
  harvest  k::grid_harvest alone over the candidates of a side-16 grid (768 planes): bytes moved (every plane read once and
           written once) over time, as a share of 8 TB/s
  paint    k::grid_paint alone, 1024 x 1024, 100 kept segments, with and without the box cull

Kernel times are means between two events on the null stream (dlimg_amd_test_grid_kernels of lib/libdlimgedit_test.so); call times are
wall clock of the calling thread, median of the repetitions after a warm-up.
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

STEPS = {"map": 420, "harvest": 180, "paint": 180}       # seconds
HBM_PEAK = 8.0e12


def _image():
    import numpy as np
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:1024, 0:1024].astype(np.float32)
    img = np.zeros((1024, 1024, 4), np.uint8)
    for c in range(3):
        img[:, :, c] = np.clip(128 + 60 * np.sin(xx * 0.01 * (c + 1)) * np.cos(yy * 0.013) + rng.uniform(-8, 8, (1024, 1024)), 0, 255).astype(np.uint8)
    img[:, :, 3] = 255
    return img


def _median_ms(call, reps):
    call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times)


def step_map():
    import numpy as np
    from dlimgedit_amd import api, weights as W
    from dlimgedit_amd.sam_config import get_config
    with tempfile.TemporaryDirectory() as d:
        W.write_synthetic_model_dir(d, get_config("vit_b"), seed=7)
        env = api.Environment(api.Options(api.Backend.gpu, d))
        seg = api.Segmentation.process(api.ImageView(_image(), api.Channels.rgba), env)
        for side in (16, 32):
            n = side * side
            pts = [api.Point((2 * i + 1) * 1024 // (2 * side), (2 * j + 1) * 1024 // (2 * side)) for j in range(side) for i in range(side)]
            outs = [np.empty((1024, 1024), np.uint8) for _ in range(n)]
            own = np.empty((1024, 1024), np.uint8)
            # thresholds that every non-empty candidate passes: synthetic weights put the predictions anywhere, and the map's cost
            # is then that of the most kept segments NMS leaves
            for ip, sp in ((-1000000, -1000000), (0, 0)):
                grid_ms, grid_min = _median_ms(lambda: seg.segment_everything(side, ip, sp, out=own), 5)
                print(f"grid.probe.map side {side} thresholds {ip}/{sp}: label map {grid_ms:.2f} ms (min {grid_min:.2f}), {int(own.max())} segments kept")
            api.ext.set_profiling(env, True)
            seg.segment_everything(side, -1000000, -1000000, out=own)
            stats = api.ext.take_stage_stats(env)
            api.ext.set_profiling(env, False)
            print(f"grid.probe.map side {side} stage clocks of one label map (ms): " +
                  ", ".join(f"{k} {v['ms']:.3f} ({v['launches']} launches)" for k, v in stats.items() if v["ms"] > 0))
            batch_ms, batch_min = _median_ms(lambda: api.Segmentation.compute_mask_batch([seg] * n, points=pts, out=outs), 3)
            print(f"grid.probe.map side {side}: batch call of {n} one-point prompts ({n} masks) {batch_ms:.2f} ms (min {batch_min:.2f})")
        seg.close()
        env.close()


def _blob_planes(prompts, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    planes4 = rng.normal(-4.0, 0.5, (prompts, 4, 256, 256)).astype(np.float32)
    for c in range(3 * prompts):
        x0, y0 = rng.integers(0, 200, 2)
        planes4[c // 3, 1 + c % 3, y0:y0 + int(rng.integers(16, 56)), x0:x0 + int(rng.integers(16, 56))] += np.float32(7.0)
    return planes4


def step_harvest():
    from dlimgedit_amd import api
    prompts = 256
    planes4 = _blob_planes(prompts)
    *_, ok, (harvest_ms, _) = api.ext.test_grid_kernels(planes4, 1024, 1024, 1024, 1024, kept=[0], time_iters=20)
    assert ok
    moved = 3 * prompts * 2 * 256 * 256 * 4
    rate = moved / (harvest_ms * 1e-3)
    print(f"grid.probe.harvest {3 * prompts} candidates in {-(-prompts // 16)} launches: {harvest_ms * 1e3:.1f} us, {moved / 1e6:.0f} MB moved, "
          f"{rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f} % of 8 TB/s")


def step_paint():
    from dlimgedit_amd import api
    planes4 = _blob_planes(34, seed=2)
    kept = list(range(100))
    for cull in (True, False):
        *_, out, _, ok, (_, paint_ms) = api.ext.test_grid_kernels(planes4, 1024, 1024, 1024, 1024, kept=kept, cull=cull, time_iters=20)
        assert ok
        print(f"grid.probe.paint 1024 x 1024, 100 kept, cull {'on' if cull else 'off'}: {paint_ms * 1e3:.1f} us, {int((out > 0).mean() * 100)} % of the pixels labelled")
    planes4 = _blob_planes(34, seed=2)
    for cull in (True, False):
        *_, out, _, ok, (_, paint_ms) = api.ext.test_grid_kernels(planes4, 600, 400, 1024, 683, kept=kept, cull=cull, time_iters=20)
        assert ok
        print(f"grid.probe.paint 600 x 400 (two stages), 100 kept, cull {'on' if cull else 'off'}: {paint_ms * 1e3:.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.step:
        {"map": step_map, "harvest": step_harvest, "paint": step_paint}[args.step]()
        return 0
    lines = []
    for step, limit in STEPS.items():
        try:
            r = subprocess.run([sys.executable, __file__, "--step", step], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"grid.probe: step {step} ran out of its {limit} s: stopping")
            return 1
        got = [l for l in r.stdout.splitlines() if l.startswith("grid.probe")]
        print("\n".join(got), flush=True)
        lines += got
        if r.returncode != 0:
            print(f"grid.probe: step {step} ended with {r.returncode}: stopping\n{r.stderr[-2000:]}")
            return 1
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
