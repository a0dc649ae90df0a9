"""The SAM-HQ tensor group dec.hq.* in the weight store: inventory, file format, name maps, the converter's path.  CPU only."""
import hashlib

import numpy as np
import pytest

import hq_cases as H
from dlimgedit_amd import weights as W
from dlimgedit_amd.sam_config import get_config

CFG = H.CFG


@pytest.fixture(scope="module")
def params():
    return W.synthetic_weights(CFG, H.SEED, mask_branch=True, hq=True)


def test_spec_lists_the_group_behind_the_decoder(params):
    plain = [n for n, _, _ in W.param_specs(CFG, True)]
    full = [n for n, _, _ in W.param_specs(CFG, True, True)]
    group = [n for n, _, _ in W.hq_specs(CFG)]
    assert full == plain + group and len(group) == 25 and all(n.startswith("dec.hq.") for n in group)
    shapes = {n: s for n, s, _ in W.hq_specs(CFG)}
    assert shapes["dec.hq.token"] == (256,) and shapes["dec.hq.mlp.2.w"] == (32, 256)
    assert shapes["dec.hq.vit.conv1.w"] == (CFG.embed_dim, 256, 2, 2) and shapes["dec.hq.vit.conv2.w"] == (256, 32, 2, 2)
    assert shapes["dec.hq.emb.conv1.w"] == (256, 64, 2, 2) and shapes["dec.hq.emb.conv2.w"] == (64, 32, 2, 2)
    assert shapes["dec.hq.mask.conv1.w"] == (64, 32, 3, 3) and shapes["dec.hq.mask.conv2.w"] == (32, 64, 3, 3)
    assert shapes["dec.hq.vit.ln.w"] == (256,) and shapes["dec.hq.emb.ln.w"] == (64,) and shapes["dec.hq.mask.ln.w"] == (64,)
    assert W.has_hq(params) and not W.has_hq(W.synthetic_weights(CFG, H.SEED))
    # the group changes no other tensor, with or without the mask branch
    for mask_branch in (False, True):
        base = W.synthetic_weights(CFG, H.SEED, mask_branch)
        with_hq = W.synthetic_weights(CFG, H.SEED, mask_branch, hq=True)
        assert set(with_hq) - set(base) == set(group)
        assert all(np.array_equal(base[k], with_hq[k]) for k in base)


@pytest.mark.parametrize("mask_branch", [False, True])
@pytest.mark.parametrize("hq", [False, True])
def test_save_and_load_round_trip(tmp_path, mask_branch, hq):
    p = W.synthetic_weights(CFG, 3, mask_branch, hq)
    path = W.save_weights(tmp_path / "m.dlw", CFG, p)
    meta, q = W.load_weights(path)
    assert meta["embed_dim"] == CFG.embed_dim and meta["global_attn_indexes"] == CFG.global_attn_indexes
    assert list(q) == [n for n, _, _ in W.param_specs(CFG, mask_branch, hq)]
    assert all(np.array_equal(p[k], q[k]) for k in p)
    assert W.has_hq(q) == hq and W.has_mask_branch(q) == mask_branch


def test_files_without_the_group_keep_their_bytes(tmp_path):
    """A file written from params without dec.hq.* is what it was before the group existed: the header, the table and the data
    are functions of param_specs(cfg, mask_branch) alone.  Pinned by the digest of the vit_test file of seed 7, which is the
    file every parity test of the suite loads."""
    cfg = get_config("vit_test")
    for mask_branch in (False, True):
        p = W.synthetic_weights(cfg, 7, mask_branch)
        a = W.save_weights(tmp_path / f"a{mask_branch}.dlw", cfg, p).read_bytes()
        # the same params with the group added and taken away again
        q = W.synthetic_weights(cfg, 7, mask_branch, hq=True)
        b = W.save_weights(tmp_path / f"b{mask_branch}.dlw", cfg, {k: v for k, v in q.items() if not k.startswith("dec.hq.")}).read_bytes()
        assert a == b
        n = len(W.param_specs(cfg, mask_branch))
        assert int.from_bytes(a[12:16], "little") == n and b"dec.hq." not in a
    assert hashlib.sha256(W.save_weights(tmp_path / "c.dlw", cfg, W.synthetic_weights(cfg, 7)).read_bytes()).hexdigest() == PLAIN_SHA256


# sha256 of sam_vit_test.dlw, seed 7, no optional group, as the parent commit writes it
PLAIN_SHA256 = "4900ca1866d025efc13bf34b86821b6f96a685a35d391cf9bd7f15192488f6ed"


def test_partial_group_is_refused(tmp_path, params):
    q = dict(params)
    del q["dec.hq.emb.ln.b"]
    with pytest.raises(ValueError, match=r"dec\.hq\.emb\.ln\.b"):
        W.has_hq(q)
    with pytest.raises(ValueError, match=r"all or nothing.*dec\.hq\.emb\.ln\.b"):
        W.save_weights(tmp_path / "m.dlw", CFG, q)
    only = {k: v for k, v in params.items() if not k.startswith("dec.hq.") or k == "dec.hq.token"}
    with pytest.raises(ValueError, match="partial SAM-HQ group"):
        W.save_weights(tmp_path / "m.dlw", CFG, only)


def test_name_maps_round_trip(params):
    for to, back, token in ((W.to_hf_state_dict, W.from_hf_state_dict, "mask_decoder.hq_token.weight"),
                            (W.to_meta_state_dict, W.from_meta_state_dict, "mask_decoder.hf_token.weight")):
        sd = to(CFG, params)
        assert sd[token].shape == (1, 256)
        q = back(CFG, sd)
        assert set(q) == set(params) and all(np.array_equal(params[k], q[k]) for k in params)
        # a state dict that lost one tensor of the group converts as plain SAM
        sd.pop(token)
        assert not W.has_hq(back(CFG, sd))
    hf, meta = W.to_hf_state_dict(CFG, params), W.to_meta_state_dict(CFG, params)
    for k in ("mask_decoder.hq_mask_mlp.proj_in.weight", "mask_decoder.hq_mask_mlp.layers.0.bias", "mask_decoder.hq_mask_mlp.proj_out.weight",
              "mask_decoder.compress_vit_conv1.weight", "mask_decoder.compress_vit_norm.bias", "mask_decoder.compress_vit_conv2.bias",
              "mask_decoder.encoder_conv1.weight", "mask_decoder.encoder_norm.weight", "mask_decoder.encoder_conv2.weight",
              "mask_decoder.mask_conv1.weight", "mask_decoder.mask_norm.weight", "mask_decoder.mask_conv2.bias"):
        assert k in hf, k
    for k in ("mask_decoder.hf_mlp.layers.0.weight", "mask_decoder.hf_mlp.layers.2.bias", "mask_decoder.compress_vit_feat.0.weight",
              "mask_decoder.compress_vit_feat.1.bias", "mask_decoder.compress_vit_feat.3.weight", "mask_decoder.embedding_encoder.0.bias",
              "mask_decoder.embedding_encoder.1.weight", "mask_decoder.embedding_encoder.3.weight",
              "mask_decoder.embedding_maskfeature.0.weight", "mask_decoder.embedding_maskfeature.1.bias",
              "mask_decoder.embedding_maskfeature.3.weight"):
        assert k in meta, k
    assert np.array_equal(hf["mask_decoder.mask_conv1.weight"], params["dec.hq.mask.conv1.w"])
    assert np.array_equal(meta["mask_decoder.embedding_maskfeature.3.weight"], params["dec.hq.mask.conv2.w"])


def test_loads_into_hugging_face_without_missing_or_unexpected_keys(params):
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    if not hasattr(transformers, "SamHQModel"):
        pytest.skip("this transformers release has no SamHQModel")
    from oracle import sam_oracle as O
    vc = transformers.SamHQVisionConfig(hidden_size=CFG.embed_dim, num_hidden_layers=CFG.depth, num_attention_heads=CFG.num_heads,
                                        global_attn_indexes=list(CFG.global_attn_indexes), mlp_dim=CFG.mlp_dim)
    dc = transformers.SamHQMaskDecoderConfig(layer_norm_eps=O.DEC_LN_EPS, vit_dim=CFG.embed_dim)
    model = transformers.SamHQModel(transformers.SamHQConfig(vision_config=vc, mask_decoder_config=dc))
    sd = {k: torch.from_numpy(np.array(v)) for k, v in W.to_hf_state_dict(CFG, params).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)


def test_f16_range_is_checked_for_the_group(tmp_path, params):
    assert W.f16_operand("dec.hq.mask.conv1.w") and W.f16_operand("dec.hq.vit.conv2.w") and W.f16_operand("dec.hq.emb.conv1.w")
    assert not W.f16_operand("dec.hq.mask.conv1.b") and not W.f16_operand("dec.hq.token") and not W.f16_operand("dec.hq.mlp.0.w")
    q = dict(params)
    q["dec.hq.mask.conv1.w"] = params["dec.hq.mask.conv1.w"].copy()
    q["dec.hq.mask.conv1.w"][3, 2, 1, 0] = 70000.0
    with pytest.raises(ValueError, match=r"dec\.hq\.mask\.conv1\.w.*f16 range"):
        W.save_weights(tmp_path / "m.dlw", CFG, q)
    W.save_weights(tmp_path / "m.dlw", CFG, q, allow_out_of_range=True)       # the escape hatch the loader's own refusal is tested with
