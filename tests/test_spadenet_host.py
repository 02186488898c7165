"""CPU (-m "not gpu"): SPADENet's constructor contract (reference: generative/networks/nets/spade_network.py) and the launch sequence of its
fused decoder, counted with the recording library of _util.conv_on_cpu (nothing is launched)."""
import importlib
import sys

import pytest
import torch

from _util import conv_on_cpu, load_fixture

CASES = ["a2d", "b3d", "c2d", "d3d"]


def _fixture():
    return load_fixture("spadenet")["cases"]


def _net(cfg, **more):
    from generativemodels_amd.networks.nets import SPADENet
    cfg = dict(cfg, **more)
    cfg["num_channels"] = list(cfg["num_channels"])
    return SPADENet(**cfg)


def test_importable_from_the_package_and_from_the_reference_path():
    import generativemodels_amd
    from generativemodels_amd.networks.nets import SPADENet
    keep = {k: v for k, v in sys.modules.items() if k == "generative" or k.startswith("generative.")}
    try:
        generativemodels_amd.install_as_generative(force=True)
        assert importlib.import_module("generative.networks.nets").SPADENet is SPADENet
        mod = importlib.import_module("generative.networks.nets.spade_network")
        for name in ("KLDLoss", "UpsamplingModes", "SPADEResNetBlock", "SPADEEncoder", "SPADEDecoder", "SPADENet"):
            assert hasattr(mod, name), name
    finally:
        for k in [k for k in sys.modules if k == "generative" or k.startswith("generative.")]:
            del sys.modules[k]
        sys.modules.update(keep)


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(name):
    fx = _fixture()[name]
    m = _net(fx["cfg"])
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(v) for k, v in fx["shapes"].items()}
    import restatement as R
    m.load_state_dict(R.synthetic_state_dict(fx["shapes"], seed=fx["synthetic_seed"]), strict=True)


def test_argument_checks_raise_the_reference_s_value_errors():
    from generativemodels_amd.networks.nets import SPADENet
    with pytest.raises(ValueError):
        SPADENet(1, 1, 8, [16, 16], [16, 32, 64, 128], 16, True)  # the reference's test_shape_wrong
    with pytest.raises(ValueError):
        SPADENet(2, 1, 1, 3, [16, 16, 16], [8, 16], 8)  # input_shape longer than spatial_dims
    with pytest.raises(ValueError):
        SPADENet(3, 1, 1, 3, [16, 16], [8, 16], 8)
    with pytest.raises(ValueError):
        SPADENet(2, 1, 1, 3, [16, 12], [8, 16, 16], 8)  # 12 is not divisible by 2 ** 3


def test_departures_from_the_reference_raise_what_the_module_says():
    cfg = _fixture()["a2d"]["cfg"]
    for mode in ("bilinear", "bicubic"):
        with pytest.raises(NotImplementedError, match=mode):
            _net(cfg, upsampling_mode=mode)
    with pytest.raises(NotImplementedError, match="BATCH"):
        _net(cfg, norm="BATCH")
    with pytest.raises(NotImplementedError, match="(?i)gelu"):
        _net(cfg, act="GELU")
    with pytest.raises(NotImplementedError, match="(?i)tanh"):
        _net(cfg, last_act="TANH")
    _net(cfg, act="RELU", last_act=None)  # none, ReLU and LeakyReLU are served
    vae = _net(cfg)
    seg = torch.zeros(2, 3, 16, 16)
    with conv_on_cpu():
        with pytest.raises(ValueError):
            vae.decode(seg, None)
    gan = _net(cfg, is_vae=False)  # constructs with the reference's parameters (fc: Linear(label_nc, ...)), cannot run -- as in the reference
    assert not hasattr(gan, "encoder") and tuple(gan.decoder.fc.weight.shape) == (16 * 4 * 4, 3)
    with conv_on_cpu():
        with pytest.raises(NotImplementedError):
            gan(seg)
        with pytest.raises(NotImplementedError):
            gan.decode(seg, torch.zeros(2, 8))


def test_the_caller_s_num_channels_list_is_left_alone():
    from generativemodels_amd.networks.nets import SPADENet
    from generativemodels_amd.networks.nets.spade_network import SPADEDecoder
    chans = [8, 8, 12]
    SPADENet(2, 2, 3, 4, [16, 24], chans, 5)
    assert chans == [8, 8, 12]
    SPADEDecoder(2, 3, 4, [16, 24], chans, 5)
    assert chans == [8, 8, 12]


# ---- the decoder's launch sequence ------------------------------------------------------------------------------------------------------------
_SB = {"x": 1, "g0": 6, "y0": 9, "g1": 11, "y1": 14, "N": 16, "src": slice(17, 20), "dst": slice(20, 23), "C": 23, "up": 24, "act": 25, "slope": 26}


def _decoder_calls(name):
    fx = _fixture()[name]
    cfg = fx["cfg"]
    m = _net(cfg).eval()
    seg = torch.zeros(2, cfg["label_nc"], *cfg["input_shape"])
    with conv_on_cpu() as rec, torch.no_grad():
        m.decode(seg, torch.zeros(2, cfg["z_dim"]))
    return m, [c for c in rec.calls if c[0] in ("gm_spade_block_apply", "gm_resample2x", "gm_spade_apply", "gm_gn_scale_shift", "gm_gn_channel_stats")]


def test_a2d_decoder_runs_two_block_applies_per_block_and_never_writes_the_upsampled_tensor():
    """a2d: blocks 16 -> 8 at 4 x 4 and 8 -> 1 at 8 x 8, both with a learned shortcut."""
    m, calls = _decoder_calls("a2d")
    assert all(b.learned_shortcut for b in m.decoder.blocks)
    applies = [c for c in calls if c[0] == "gm_spade_block_apply"]
    assert len(applies) == 4 and not [c for c in calls if c[0] in ("gm_resample2x", "gm_spade_apply")]
    first0, second0, first1, second1 = applies
    # block 0: the grid it was given; one pass writes norm_0 + LeakyReLU(0.2) and norm_s
    assert first0[_SB["up"]] == 0 and first0[_SB["src"]] == [1, 4, 4] == first0[_SB["dst"]] and first0[_SB["C"]] == 16
    assert first0[_SB["g0"]] and first0[_SB["g1"]] and first0[_SB["y1"]] and first0[_SB["act"]] == 3 and first0[_SB["slope"]] == pytest.approx(0.2)
    assert second0[_SB["up"]] == 0 and second0[_SB["C"]] == 8 and second0[_SB["g0"]] and not second0[_SB["g1"]] and not second0[_SB["y1"]]
    # block 1 reads block 0's 4 x 4 output through the up-sampling
    assert first1[_SB["up"]] == 1 and first1[_SB["src"]] == [1, 4, 4] and first1[_SB["dst"]] == [1, 8, 8] and first1[_SB["C"]] == 8
    assert first1[_SB["g1"]] and first1[_SB["y1"]]
    assert second1[_SB["up"]] == 0 and second1[_SB["C"]] == 1 and second1[_SB["dst"]] == [1, 8, 8] and not second1[_SB["g1"]]
    # block 1's statistics are those of block 0's 4 x 4 output (16 voxels, 8 channels): no pass over the 64 voxels of its up-sampling
    stats = [(c[4], c[5]) for c in calls if c[0] == "gm_gn_channel_stats"]
    assert (16, 8) in stats and (64, 8) not in stats and not [c for c in calls if c[0] == "gm_gn_scale_shift"]


def test_d3d_decoder_materialises_the_upsampling_only_for_an_identity_shortcut():
    """d3d: blocks 16 -> 16 (identity shortcut, at 4 x 2 x 6) and 16 -> 2 (learned, through the up-sampling, at 8 x 4 x 12)."""
    m, calls = _decoder_calls("d3d")
    assert [b.learned_shortcut for b in m.decoder.blocks] == [False, True]
    applies = [c for c in calls if c[0] == "gm_spade_block_apply"]
    assert len(applies) == 4
    assert [c[_SB["up"]] for c in applies] == [0, 0, 1, 0]
    assert [bool(c[_SB["g1"]]) for c in applies] == [False, False, True, False]
    assert applies[2][_SB["src"]] == [4, 2, 6] and applies[2][_SB["dst"]] == [8, 4, 12]
    assert not [c for c in calls if c[0] == "gm_resample2x"]  # block 0's identity residual is x itself; the last convolution folds its up-sampling


def test_c2d_identity_shortcut_behind_an_upsampling_is_the_one_resample_call():
    """c2d: 12 -> 8 (learned), 8 -> 8 (identity, through the up-sampling: its residual up(x) is materialised), 8 -> 3 (learned)."""
    m, calls = _decoder_calls("c2d")
    assert [b.learned_shortcut for b in m.decoder.blocks] == [True, False, True]
    applies = [c for c in calls if c[0] == "gm_spade_block_apply"]
    assert [c[_SB["up"]] for c in applies] == [0, 0, 1, 0, 1, 0]
    assert [bool(c[_SB["g1"]]) for c in applies] == [True, False, False, False, True, False]
    assert len([c for c in calls if c[0] == "gm_resample2x"]) == 1
