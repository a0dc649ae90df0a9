"""The SAM-HQ feature branch as the product's encoder runs it (SamModel::hq_branch: a transposed convolution as a GEMM, the row
LayerNorm with GELU and an f16-only result on [M][4 C] read as [4 M][C], a second GEMM with K = C; then k::hq_features_finish),
through ext.test_hq_branch: lane 0 of a SAM-HQ model's environment, the entry SamModel::encode calls, on a given f16 input.

Every stage is computed from the operands that stage had on the device (teacher forcing) against the float64 reference of
tests/hq_feature_ref.py: A from the input and the loaded W1 / b1, H from the delivered A, Y from the delivered H.  The allowance is
ALLOW = 1.25 times the larger numpy fp32 yardstick on the same inputs, whole tensors throughout (GEMMs: chain / trunc16 through
gemm_ref.check; LayerNorm: row_ref's three), H half an f16 spacing on top.  The loaded operands are compared with
the raw tensors element for element.  Only the finished features are compared free-running, at 3 times the distance between the
float64 and the float32 emulation.  tests/test_hq_feature_ref.py shows what these measures reject.

Models: hq_cases' geometry (D = 128: two K steps in the ViT branch's first GEMM) and one with D = 320 (five), each also with 40
added to both conv1 biases for the offset rows (hq_feature_ref.offset_params).  The 4096 tokens per image are fixed by the hook;
one image is the smallest launch.

Through the handle: the embedding half is fed with the handle's own embedding rounded to f16.  The ViT half has no tap behind a
pass (its input buffer is reused), so its input is the f16 stream of a depth-1 twin (the same weights cut behind the first
global block, block 0 of this geometry); the twin's pass may choose other GEMM tiles than the handle's, so that comparison is
held to the free-running allowance, not to bits.

Measured on MI355X (48 tests, 18 s; rms / max in units of the fp32 rounding model, "allowed" 1.25 times the larger yardstick; every
figure is in parity_margins.txt, the same table in LABNOTES.md):

                                                              kernel                     larger yardstick           allowed
    A, ViT branch, Gaussian, D = 128                          3.15 / 4.01                8.70 / 11.5                10.9 / 14.4
    A, ViT branch, Gaussian, D = 320                          4.67 / 6.34                20.3 / 16.7                25.4 / 20.8
    A, ViT branch, spike, D = 128 / 320                       3.20 / 3.84, 4.76 / 4.14   8.78 / 38.6, 20.6 / 23.5   11.0 / 48.2, 25.8 / 29.4
    A, embedding branch, Gaussian / spike                     4.21 / 4.91, 4.05 / 1.68   16.4 / 14.9, 16.2 / 14.1   20.5 / 18.6, 20.2 / 17.6
    A, offset rows (all four)                                 1.000 / 1.039              1.001 / 1.109              1.25 / 1.39
    H (f16) error / bound: Gaussian, spike, offset (worst)    0.998, 0.997, 0.806                                   1
    Y, ViT branch (K = 256), worst of six                     4.14 / 8.71                16.6 / 22.2                20.7 / 27.7
    Y, embedding branch (K = 64), worst of three              2.29 / 3.65                5.40 / 11.5                6.75 / 14.3
    features free-running, max abs, D = 128 / 320             4.23e-4 / 4.23e-4          emulations apart 4.22e-4   1.27e-3
    handle: ViT half vs the hook on the twin's stream         3.2e-7                     emulations apart 2.1e-4    6.4e-4
    handle: hq_features vs the hook chain                     0                                                     6.4e-4
    loader: differing elements                                0                                                     0

The embedding branch's tensors depend on the seed and their names alone, so its D = 320 cases repeat the D = 128 ones bit for bit.
"""
import numpy as np
import pytest

import hq_cases as H
import hq_feature_ref as F
import hq_kernel_ref as HK
from conftest import within

pytestmark = pytest.mark.gpu

f16, f32, f64 = np.float16, np.float32, np.float64

GEOMETRIES = ("d128", "d320")
BRANCHES = ("vit", "emb")
CASES = [(g, b, k) for g in GEOMETRIES for b in BRANCHES for k in F.KINDS]
IDS = ["-".join(c) for c in CASES]


def _config(geometry):
    from dlimgedit_amd.sam_config import SamConfig
    return H.CFG if geometry == "d128" else SamConfig("vit_hqtest320", 320, 2, 4, (1,))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == f16 else np.uint32)


class Models:
    """Per geometry the HQ model and its offset variant: directories, raw tensors, environments; the hook's runs, cached."""

    def __init__(self, api, tmp_path_factory):
        from dlimgedit_amd import weights as W
        self.api, self.ext = api, api.ext
        self.params, self.envs, self.cache = {}, {}, {}
        for g in GEOMETRIES:
            cfg = _config(g)
            base = W.synthetic_weights(cfg, H.SEED, hq=True)
            for variant, params in (("base", base), ("offset", F.offset_params(base))):
                d = tmp_path_factory.mktemp(f"hqfeat_{g}_{variant}")
                W.save_weights(d / "segmentation" / W.weight_file_name(cfg), cfg, params)
                self.params[g, variant] = params
                self.envs[g, variant] = api.Environment(api.Options(api.Backend.gpu, str(d)))

    @staticmethod
    def variant(kind):
        return "offset" if kind == "offset" else "base"

    def operands(self, g, variant, branch):
        """What the loader left on the device (the hook returns it with every run: any run's will do)."""
        return {k: self.run(g, branch, "offset" if variant == "offset" else "gaussian")[k] for k in F.OPERANDS}

    def run(self, g, branch, kind):
        key = (g, branch, kind)
        if key not in self.cache:
            env = self.envs[g, self.variant(kind)]
            # the input is built from the loader's model of the operands; test_loader_* holds the device's to the same values
            ops = F.loader_operands(self.params[g, self.variant(kind)], branch)
            a = F.branch_input(kind, 900 + 10 * BRANCHES.index(branch) + F.KINDS.index(kind), ops)
            out = self.ext.test_hq_branch(env, branch, a)
            out["a"] = a
            self.cache[key] = out
        return self.cache[key]

    def close(self):
        for env in self.envs.values():
            env.close()


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from dlimgedit_amd import api
    assert api.ext.device_count() >= 1, "no HIP device visible"
    m = Models(api, tmp_path_factory)
    yield m
    m.close()


# ------------------------------------------------------------------------------------------ loader

@pytest.mark.parametrize("g", GEOMETRIES)
@pytest.mark.parametrize("variant", ["base", "offset"])
def test_loader_permutes_rounds_and_repeats(models, g, variant):
    """The loaded operands of both branches against the raw tensors: the convolution weights are round_f16 of the tensor permuted
    to row = sub-pixel * co + channel with sub-pixel s = ky * 2 + kx, the biases are repeated four times, the norms are unchanged.
    No differing element is allowed; the exchanged sub-pixel order differs in nearly half of the rows."""
    for branch in BRANCHES:
        dev = models.operands(g, variant, branch)
        want = F.loader_operands(models.params[g, variant], branch)
        for k in F.OPERANDS:
            assert dev[k].dtype == want[k].dtype and dev[k].shape == want[k].shape, (branch, k)
            differing = int((_bits(dev[k]) != _bits(want[k])).sum())
            within(f"hq features loader {g} {variant} {branch} {k} differing elements", differing, 1)
        wrong = F.loader_operands(models.params[g, variant], branch, order="xy")
        assert (_bits(dev["w1"]) != _bits(wrong["w1"])).any(axis=1).mean() > 0.45
        assert (_bits(dev["w2"]) != _bits(wrong["w2"])).any(axis=1).mean() > 0.45


# ------------------------------------------------------------------------------------------ the three stages, teacher-forced

@pytest.mark.parametrize("g,branch,kind", CASES, ids=IDS)
def test_stage_a_first_gemm(models, g, branch, kind):
    """A [4096][4 C] against plain(a, W1, b1) from the device's own W1 and b1; the input's conditions are asserted on that reference."""
    r = models.run(g, branch, kind)
    F.input_conditions(kind, F.stage_a(r["a"], r), r)
    F.check_gemm(f"hq features {g} {branch} {kind} A", r["A"], r["a"], r["w1"], r["b1"])


@pytest.mark.parametrize("g,branch,kind", CASES, ids=IDS)
def test_stage_h_layernorm_gelu_f16(models, g, branch, kind):
    """H [16384][C] against float64 GELU(LN(A delivered, read as [16384][C])), eps 1e-6, biased variance, element by element."""
    r = models.run(g, branch, kind)
    assert r["H"].shape == (4 * F.TOKENS, F.BRANCHES[branch][1])
    F.check_h(f"hq features {g} {branch} {kind} H", r["H"], r["A"], r)


@pytest.mark.parametrize("g,branch,kind", CASES, ids=IDS)
def test_stage_y_second_gemm(models, g, branch, kind):
    """Y [16384][128] against plain(H delivered, W2), no bias: K = 256 (ViT branch, four K steps) or 64 (embedding branch, one)."""
    r = models.run(g, branch, kind)
    assert r["w2"].shape[1] == (256 if branch == "vit" else 64)
    F.check_gemm(f"hq features {g} {branch} {kind} Y", r["Y"], r["H"], r["w2"])


# ------------------------------------------------------------------------------------------ the finished features, free-running

@pytest.mark.parametrize("g", GEOMETRIES)
def test_features_free_running(models, g):
    """k::hq_features_finish on the two delivered Y against the float64 emulation of both branches from their inputs and the
    device's operands (f16 weights, H rounded to f16): within 3 times the largest distance between that emulation in float64
    and in float32, the allowance for two independent draws of f16-boundary flips in H.  Both numbers are logged."""
    vit, emb = models.run(g, "vit", "gaussian"), models.run(g, "emb", "gaussian")
    got, ok = models.ext.test_hq_features_finish(vit["Y"], emb["Y"], vit["b2"][:32], emb["b2"][:32])
    assert ok, "a guard byte around a device buffer was overwritten"
    e64 = F.emulate(vit["a"], emb["a"], vit, emb)
    e32 = F.emulate(vit["a"], emb["a"], vit, emb, ft=f32)
    yard = float(np.abs(e64 - e32).max())
    within(f"hq features {g} free-running emulation float64 vs float32 max abs", yard, np.inf)
    within(f"hq features {g} free-running features vs emulation max abs", np.abs(got.astype(f64) - e64).max(), 3 * yard)


# ------------------------------------------------------------------------------------------ batch, refusals

@pytest.mark.parametrize("g", GEOMETRIES)
@pytest.mark.parametrize("branch", BRANCHES)
def test_two_images_equal_each_alone(models, g, branch):
    """B = 2 with two different inputs: each image's A, H and Y are the bits of its own B = 1 call."""
    one, two = models.run(g, branch, "gaussian"), models.run(g, branch, "spike")
    assert not np.array_equal(one["a"], two["a"])
    both = models.ext.test_hq_branch(models.envs[g, "base"], branch, np.concatenate([one["a"], two["a"]]))
    for k, per in (("A", F.TOKENS), ("H", 4 * F.TOKENS), ("Y", 4 * F.TOKENS)):
        assert both[k].shape[0] == 2 * per
        assert np.array_equal(_bits(both[k][:per]), _bits(one[k])), (k, 0)
        assert np.array_equal(_bits(both[k][per:]), _bits(two[k])), (k, 1)


@pytest.fixture(scope="module")
def twin(models, tmp_path_factory):
    """The plain depth-1 twin of the D = 128 model: the same weights cut behind block 0, the first global block; no dec.hq.*."""
    from dlimgedit_amd import weights as W
    from dlimgedit_amd.sam_config import SamConfig
    assert H.CFG.global_attn_indexes[0] == 0
    cfg = SamConfig("vit_hqtest_d1", H.CFG.embed_dim, 1, H.CFG.num_heads, (0,))
    params = {k: v for k, v in models.params["d128", "base"].items() if not k.startswith("dec.hq.")}
    d = tmp_path_factory.mktemp("hqfeat_twin")
    W.save_weights(d / "segmentation" / W.weight_file_name(cfg), cfg, params)
    env = models.api.Environment(models.api.Options(models.api.Backend.gpu, str(d)))
    yield env
    env.close()


def test_refusals_launch_nothing(models, twin):
    api, ext = models.api, models.ext
    env = models.envs["d128", "base"]
    a = models.run("d128", "emb", "gaussian")["a"]
    with pytest.raises(api.Error, match="not a SAM-HQ model"):
        ext.test_hq_branch(twin, "emb", a)
    for batch in (0, 3, -1):
        with pytest.raises(api.Error, match="a call takes 1 or 2 images"):
            ext.test_hq_branch(env, "emb", np.concatenate([a, a, a]), batch=batch)
    with pytest.raises(api.Error, match="null pointer"):
        ext.test_hq_branch(env, "emb", None, batch=1)
    with pytest.raises(api.Error, match="branch is 0"):
        ext.test_hq_branch(env, 2, a)
    again = ext.test_hq_branch(env, "emb", a)
    assert np.array_equal(_bits(again["Y"]), _bits(models.run("d128", "emb", "gaussian")["Y"]))


# ------------------------------------------------------------------------------------------ through the handle

def test_handle_features_are_the_hook_chain(models, twin):
    """One image through Segmentation.process on the D = 128 model; decoder_state's hq_features against the hook chain.  The
    embedding half gets the handle's own embedding rounded to f16; what is left of the handle's features once that half and both
    biases are taken off is the ViT half, compared with the ViT branch run on the twin's f16 stream (the module's docstring):
    within 3 times the float64 / float32 distance of that branch's emulation plus the three fp32 adds of the finish."""
    api, ext = models.api, models.ext
    env = models.envs["d128", "base"]
    img = H.image("square")
    seg = api.Segmentation.process(api.ImageView(img, api.Channels.rgba), env)
    try:
        feat = ext.decoder_state(seg, api.Point(*H.CASES[0][1][0]))["hq_features"].reshape(256, 256, 32)
        emb16 = ext.get_embedding(seg).reshape(F.TOKENS, 256).astype(f16)
    finally:
        seg.close()
    stream16 = ext.test_encoder_state(twin, [img])["stream_hi"].reshape(F.TOKENS, H.CFG.embed_dim).astype(f16)
    emb, vit = ext.test_hq_branch(env, "emb", emb16), ext.test_hq_branch(env, "vit", stream16)
    chain, ok = ext.test_hq_features_finish(vit["Y"], emb["Y"], vit["b2"][:32], emb["b2"][:32])
    assert ok
    zero = np.zeros_like(emb["Y"])
    vit_half = feat.astype(f64) - HK.finish(zero, emb["Y"], vit["b2"][:32], emb["b2"][:32])
    want = HK.finish(vit["Y"], zero, np.zeros(32), np.zeros(32))
    e64 = F.emulate_branch(stream16, vit)
    e32 = F.emulate_branch(stream16, vit, ft=f32)
    yard = float(np.abs(e64 - e32.astype(f64)).max())
    rounding = float(HK.finish_bound(vit["Y"], emb["Y"], vit["b2"][:32], emb["b2"][:32]).max())
    within("hq features handle: ViT branch emulation float64 vs float32 max abs", yard, np.inf)
    within("hq features handle: ViT half vs the hook on the twin's stream max abs", np.abs(vit_half - want).max(), 3 * yard + rounding)
    within("hq features handle: features vs the hook chain max abs", np.abs(feat.astype(f64) - chain.astype(f64)).max(),
           3 * yard + rounding)
