"""Measurements of the prior mark (a caller's mask as SAM's mask input), ViT-B synthetic weights with the mask branch.

    python tools/prior_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::mask_prior alone at 1024 x 1024 and 4000 x 3000 (dlimg_amd_test_prior_plane of lib/libdlimgedit_test.so):
           microseconds per launch and bytes moved (the mask read once, the plane written once) over time, as a share of 8 TB/s
  query    a one-click query with a prior against the same query without one, on one 1024 x 1024 and one 4000 x 3000 image:
           wall clock of the calling thread (median and minimum of the repetitions after a warm-up) and, with the stage clocks
           on, the milliseconds and launches of the decoder stage and of stage 7 (post: this kernel and the post-processing)

Kernel times are means between two events on the null stream; the prior is a numpy array of the caller's (the staging road).
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

STEPS = {"kernel": 180, "query": 300}       # seconds
HBM_PEAK = 8.0e12
EXTENTS = [(1024, 1024), (4000, 3000)]


def _image(w, h):
    import numpy as np
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.zeros((h, w, 4), np.uint8)
    for c in range(3):
        img[:, :, c] = np.clip(128 + 60 * np.sin(xx * 0.01 * (c + 1)) * np.cos(yy * 0.013) + rng.uniform(-8, 8, (h, w)), 0, 255).astype(np.uint8)
    img[:, :, 3] = 255
    return img


def _ellipse(w, h):
    import numpy as np
    yy, xx = np.mgrid[0:h, 0:w]
    return np.where(((xx - 0.5 * w) / (0.3 * w)) ** 2 + ((yy - 0.5 * h) / (0.25 * h)) ** 2 <= 1, 255, 0).astype(np.uint8)


def step_kernel():
    from dlimgedit_amd import api
    for w, h in EXTENTS:
        scale = 1024 / max(w, h)
        pre_w, pre_h = int(w * scale + 0.5), int(h * scale + 0.5)
        mask = _ellipse(w, h)
        api.ext.test_prior_plane(mask, pre_w, pre_h, 8000, time_iters=20)          # warm-up
        _, ok, ms = api.ext.test_prior_plane(mask, pre_w, pre_h, 8000, time_iters=200)
        moved = w * h + 256 * 256 * 4
        print(f"kernel {w}x{h}: {ms * 1e3:.2f} us per launch, {moved} bytes: {moved / (ms * 1e-3) / 1e12:.3f} TB/s = "
              f"{100 * moved / (ms * 1e-3) / HBM_PEAK:.1f} % of 8 TB/s; guards intact {ok}")


def step_query():
    from dlimgedit_amd import api, weights as W
    from dlimgedit_amd.sam_config import get_config
    with tempfile.TemporaryDirectory() as d:
        W.write_synthetic_model_dir(d, get_config("vit_b"), seed=7, mask_branch=True)
        env = api.Environment(api.Options(api.Backend.gpu, d))
        for w, h in EXTENTS:
            seg = api.Segmentation.process(api.ImageView(_image(w, h), api.Channels.rgba), env)
            prior, out = _ellipse(w, h), api._mask_image(seg.extent())
            click = [api.Point(w // 2, h // 2)]
            for name, kw in (("without", {}), ("with a prior", {"prior": prior})):
                call = lambda: seg.compute_mask_clicks(click, out=out, **kw)     # noqa: E731
                for _ in range(5):
                    call()
                times = []
                for _ in range(50):
                    t0 = time.perf_counter()
                    call()
                    times.append((time.perf_counter() - t0) * 1e3)
                api.ext.set_profiling(env, True)
                api.ext.take_stage_stats(env)
                for _ in range(20):
                    call()
                st = api.ext.take_stage_stats(env)
                api.ext.set_profiling(env, False)
                print(f"query {w}x{h} {name}: wall median {statistics.median(times):.3f} ms, min {min(times):.3f} ms; per query decoder "
                      f"{st['decoder']['ms'] / 20:.4f} ms in {st['decoder']['launches'] / 20:g} timed spans, post {st['post']['ms'] / 20:.4f} ms in "
                      f"{st['post']['launches'] / 20:g} launches, {st['post']['work'] / 20:.0f} bytes")
            seg.close()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        {"kernel": step_kernel, "query": step_query}[args.step]()
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
