"""Measurements of the lasso mark (a selection snapped to the object: box and click derived on the GPU), ViT-B synthetic
weights with the mask branch.

    python tools/lasso_probe.py [--out FILE]

Steps, each a fresh child process under its own time limit; the first one that fails, is killed or runs out of time ends the
run (nothing more is started on the GPU after it):
  kernel   k::lasso_derive alone (both launches, behind a plane k::mask_prior wrote; dlimg_amd_test_lasso_derive of
           lib/libdlimgedit_test.so) at 1024 x 1024, 1800 x 1200 and 4000 x 3000: microseconds per derivation, for an
           ellipse and for a full selection (the longest column scans and the largest distances)
  query    a lasso-only call (what = 0: box, click and mask input) against the SAME prompt sent explicitly -- the reference's
           box and click (tests/lasso_ref.py) and a prior mark on the same buffer -- on one image of each extent: wall clock of
           the calling thread (median and minimum of the repetitions after a warm-up) and, with the stage clocks on, the
           milliseconds and launches of the decoder stage and of stage 7 (post: mask_prior, the derive launches and the
           post-processing).  `--explicit-only` times the explicit call alone, which also runs on a build without the mark.

Kernel times are means between two events on the null stream; the selection is a numpy array of the caller's (the staging road).
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
EXTENTS = [(1024, 1024), (1800, 1200), (4000, 3000)]


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


def _pre(w, h):
    scale = 1024 / max(w, h)
    return (w, h) if max(w, h) == 1024 else (int(w * scale + 0.5), int(h * scale + 0.5))


def step_kernel():
    import numpy as np
    from dlimgedit_amd import api
    for w, h in EXTENTS:
        pre_w, pre_h = _pre(w, h)
        for name, mask in (("ellipse", _ellipse(w, h)), ("full", np.full((h, w), 255, np.uint8))):
            api.ext.test_lasso_derive(mask, pre_w, pre_h, time_iters=20)          # warm-up
            rec, ok, ms = api.ext.test_lasso_derive(mask, pre_w, pre_h, time_iters=200)
            print(f"kernel {w}x{h} {name}: {ms * 1e3:.2f} us per derivation (2 launches), record {rec.tolist()}; guards intact {ok}")


def step_query(explicit_only=False):
    import lasso_ref
    from dlimgedit_amd import api, weights as W
    from dlimgedit_amd.sam_config import get_config
    with tempfile.TemporaryDirectory() as d:
        W.write_synthetic_model_dir(d, get_config("vit_b"), seed=7, mask_branch=True)
        env = api.Environment(api.Options(api.Backend.gpu, d))
        for w, h in EXTENTS:
            seg = api.Segmentation.process(api.ImageView(_image(w, h), api.Channels.rgba), env)
            sel, out = _ellipse(w, h), api._mask_image(seg.extent())
            rec = lasso_ref.derive(sel, *_pre(w, h))
            click = [api.Point(int(rec[5]), int(rec[6]))]
            box = api.Region(api.Point(int(rec[1]), int(rec[2])), api.Point(int(rec[3]), int(rec[4])))
            calls = [("explicit (box, click, prior mark)", lambda: seg.compute_mask_clicks(click, None, box, out=out, prior=sel))]
            if not explicit_only:
                calls.append(("lasso mark", lambda: seg.snap_selection(sel, out=out)))
            masks = []
            for name, call in calls:
                for _ in range(5):
                    call()
                masks.append(out.copy())
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
            if len(masks) == 2:
                print(f"query {w}x{h}: the two masks are byte-equal: {bool((masks[0] == masks[1]).all())}")
            seg.close()
        env.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--step", choices=sorted(STEPS))
    ap.add_argument("--explicit-only", action="store_true")
    args = ap.parse_args()
    if args.step:
        step_kernel() if args.step == "kernel" else step_query(args.explicit_only)
        return 0
    lines = []
    for step, limit in STEPS.items():
        if step == "kernel" and args.explicit_only:
            continue
        cmd = [sys.executable, __file__, "--step", step] + (["--explicit-only"] if args.explicit_only else [])
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
