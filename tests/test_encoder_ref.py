"""CPU checks of tests/encoder_ref.py, the reference tests/test_gpu_encoder.py holds the encoder chain to.

Sensitivity: every stand-in below is a MODIFIED chain or fold -- a shortcut or a slip the product could make without the
end-to-end tolerance noticing -- and must fail the staged check it targets, with the GPU file's own bound on the GPU file's
own inputs (d512, the sinusoid image, the emulated device values), by at least 3 x the bound.  Next to it the log receives the
stand-in's free-running embedding error beside EMB_TOL, the tolerance the full-size end-to-end test samples the embedding
with, and beside the GPU file's free-running bound (3 x the emulation's float64-to-float32 distance), with a note where it is not
3 x that bound: recorded, not asserted -- it shows which of them only the staged checks catch.

Also pinned: weights are drawn by name, so a model of depth k holds exactly the first k blocks of a deeper one (what the GPU
file's prefix models rely on), and every reference qkv and hidden stays inside the f16 range."""
import numpy as np
import pytest

import encoder_cases as C
import encoder_ref as E
import gemm_ref as G
from conftest import EMB_TOL, at_least, within

GEOMETRY = "d512"
CAUGHT = 3.0        # a stand-in's worst value / bound


@pytest.fixture(scope="module")
def chain():
    """kind -> the emulated device values of the unmodified chain on the sinusoid image."""
    cache = {}

    def get(kind: str):
        if kind not in cache:
            cfg = C.config(GEOMETRY)
            params = C.parameters(GEOMETRY, kind)
            patches = E.patches_from_image(C.image("sinusoids"))
            outer = E.outer_model(params)
            layers = [E.loader_model(E.fold64(params, cfg, j)) for j in range(cfg.depth)]
            run = E.emulate(patches, outer, layers, cfg)
            # the GPU file's free-running bound: 3 x the distance between the emulation in float64 and in float32
            yard = float(np.abs(run["embedding"] - E.emulate(patches, outer, layers, cfg, ft=np.float32)["embedding"]).max())
            within(f"free-running emulation float64 vs float32 max abs, {kind} weights", yard, np.inf)
            cache[kind] = {"free_running_bound": 3 * yard, "cfg": cfg, "params": params, "patches": patches, "outer": outer, "layers": layers, "run": run,
                           "rows": E.yardstick_rows(C.YARDSTICK_ROWS, patches)}
        return cache[kind]

    return get


@pytest.mark.parametrize("geometry", sorted(C.GEOMETRIES))
@pytest.mark.parametrize("kind", sorted(C.SEEDS))
def test_a_shallower_model_is_a_prefix_of_the_deeper_one(geometry, kind):
    """Depth 1 has no global block at all; the tensors outside the blocks do not depend on the depth either."""
    full = C.parameters(geometry, kind)
    for depth in range(1, C.GEOMETRIES[geometry][1]):
        cfg = C.config(geometry, depth)
        assert cfg.global_attn_indexes == tuple(g for g in C.GEOMETRIES[geometry][3] if g < depth)
        part = C.parameters(geometry, kind, depth)
        assert set(part) < set(full) and not [n for n in full if n not in part and not n.startswith(f"enc.L")]
        for name, value in part.items():
            assert np.array_equal(value, full[name]), (depth, name)


@pytest.mark.parametrize("kind", sorted(C.SEEDS))
def test_references_stay_in_the_f16_range(chain, kind):
    c = chain(kind)
    for j, (taps, L) in enumerate(zip(c["run"]["blocks"], c["layers"])):
        x = taps["stream_in"][0] + taps["stream_in"][1]
        qkv = G.consumer(taps["stream_in"][0], L["qkv.w"], L["qkv.colsum"], L["qkv.b"], x)
        mid = taps["x_mid"][0] + taps["x_mid"][1]
        hidden = G.consumer(taps["x_mid"][0], L["fc1.w"], L["fc1.colsum"], L["fc1.b"], mid, act=1)
        assert np.abs(qkv).max() < G.F16_LIMIT and np.abs(hidden).max() < G.F16_LIMIT, (kind, j)
        assert np.array_equal(G.round_f16(qkv), taps["qkv"]) and np.array_equal(G.round_f16(hidden), taps["hidden"])


def test_the_unmodified_chain_passes_its_own_checks(chain):
    """The last block's stages, the neck and every fold check on the emulation itself: all within their bounds."""
    c = chain("synthetic")
    cfg, rows, j = c["cfg"], c["rows"], c["cfg"].depth - 1
    taps, L = c["run"]["blocks"][j], c["layers"][j]
    measures = E.stage0("ref S0", c["run"]["blocks"][0]["stream_in"], c["patches"], c["outer"], rows)
    measures += E.consumer_stage("ref S1", taps["qkv"], taps["stream_in"], L, "qkv", 0, rows)
    measures += E.stage2("ref S2", taps["x_mid"], taps["qkv"], taps["stream_in"], L, cfg, rows)
    measures += E.consumer_stage("ref S3", taps["hidden"], taps["x_mid"], L, "fc1", 1, rows, resplit=True)
    measures += E.stage4("ref S4", taps["stream_out"], taps["hidden"], taps["x_mid"], L, rows)
    measures += E.stage5("ref S5", c["run"]["embedding"].astype(np.float32), taps["stream_out"][0], c["outer"], rows)
    measures += E.outer_measures("ref fold outer", c["outer"], c["params"])
    for i, ops in enumerate(c["layers"]):
        measures += E.fold_measures(f"ref fold block{i}", ops, c["params"], cfg, i)
    E.hold(measures)


# (stand-in, weights, block it is applied at): chain stand-ins are encoder_ref.EMULATION_VARIANTS, fold stand-ins FOLD_VARIANTS
STAND_INS = [("writer_hi_only", "synthetic", 1), ("proj_resid_hi_only", "trained", 2), ("stats_from_f16", "trained", 2),
             ("no_beta", "synthetic", 0), ("tables_unscaled", "synthetic", 1), ("q_bias_unscaled", "synthetic", 1),
             ("k_scaled", "synthetic", 1), ("pad_zero", "synthetic", 2), ("gelu_tanh", "synthetic", 2),
             ("neck_tap_order", "synthetic", 2)]


@pytest.mark.parametrize("stand_in,kind,at", STAND_INS)
def test_stand_in_fails_the_staged_check_it_targets(chain, stand_in, kind, at):
    c = chain(kind)
    cfg, rows, base = c["cfg"], c["rows"], c["run"]["blocks"][at]
    layers = list(c["layers"])
    if stand_in in E.FOLD_VARIANTS:
        layers[at] = E.loader_model(E.fold64(c["params"], cfg, at, stand_in))
        measures = E.fold_measures(f"stand-in {stand_in} fold block{at}", layers[at], c["params"], cfg, at)
        run = E.emulate(c["patches"], c["outer"], layers, cfg, start=(at, base["stream_in"]))
    else:
        run = E.emulate(c["patches"], c["outer"], layers, cfg, variant=stand_in, at=at, start=(at, base["stream_in"]))
        mine, L, name = run["blocks"][0], layers[at], f"stand-in {stand_in} block{at}"
        if stand_in == "writer_hi_only":
            measures = E.stage4(name, mine["stream_out"], base["hidden"], base["x_mid"], L, rows)
        elif stand_in == "proj_resid_hi_only":
            measures = E.stage2(name, mine["x_mid"], base["qkv"], base["stream_in"], L, cfg, rows)
        elif stand_in == "stats_from_f16":
            measures = E.consumer_stage(name, mine["qkv"], base["stream_in"], L, "qkv", 0, rows)
        elif stand_in == "gelu_tanh":
            measures = E.consumer_stage(name, mine["hidden"], base["x_mid"], L, "fc1", 1, rows, resplit=True)
        else:
            assert stand_in == "neck_tap_order"
            measures = E.stage5(name, run["embedding"], base["stream_out"][0], c["outer"], rows)
    for m in measures:
        print(m)
    worst = E.worst(measures)
    at_least(f"stand-in {stand_in}: worst value / bound of the staged check", min(worst, 1e30), CAUGHT)
    distance = np.abs(run["embedding"] - c["run"]["embedding"]).max()
    within(f"stand-in {stand_in}: free-running embedding error (EMB_TOL {EMB_TOL:g}: "
           f"{'lets it through' if distance < EMB_TOL else 'catches it'})", distance, np.inf)
    bound = c["free_running_bound"]
    seen = "at least 3 x the free-running bound" if distance >= 3 * bound else \
        "NOT 3 x the free-running bound: only the staged check catches it"
    within(f"stand-in {stand_in}: free-running embedding error / free-running bound {bound:.3g} ({seen})", distance / bound, np.inf)
