"""The launch geometry that ops.ConvGeom derives from the nn.Conv1d / nn.ConvTranspose1d containers of
ConvAutoencoder and ConvReconstruction, against the numbers their conv_gemm / wgrad call sites stated by hand
before the layers were described once: forward, data gradient, weight gradient and the pack plan."""
import pytest
import torch.nn as nn

from speech_anonymization_amd import ops
from speech_anonymization_amd._lib import SaHipError
from speech_anonymization_amd.convae import ConvAutoencoder
from speech_anonymization_amd.endtoend import ConvReconstruction

T = "sex_classifier.tdnn."
C5, D5 = ops.taps_conv(5, 1, 2), ops.taps_conv_dgrad_s1(5, 1, 2)          # the k5 p2 stride-1 tables
W5 = [(-2, 0), (-1, 0), (0, 0), (1, 0), (2, 0)]
WT = [(1, 0), (1, 1), (0, 0), (0, 1), (-1, 0)]                              # the parent's CONVT_WG_TAPS


@pytest.fixture(scope="module")
def lay():
    return ConvAutoencoder().lay, ConvReconstruction().lay


def convae_tables(Ltot):
    """{layer: (Lin, fwd, dgrad, wgrad)} as the call sites of the ConvAutoencoder step had them"""
    L2, L4 = Ltot // 2, Ltot // 4
    La, Lb, Lc = L4 - 4, L4 - 8, L4 - 14
    s1_128 = (L4, (128, 128, 1, 1, C5, L4), (128, 128, 1, 1, D5, L4), (128, 128, 1, 1, W5, L4, (5, 640, 1)))
    s1_64 = (L2, (64, 64, 1, 1, C5, L2), (64, 64, 1, 1, D5, L2), (64, 64, 1, 1, W5, L2, (5, 320, 1)))
    return {
        "encoder.2": (Ltot, (32, 64, 2, 1, C5, L2), (64, 32, 1, 2, ops.UP2, Ltot), (32, 64, 2, 1, W5, L2, (5, 160, 1))),
        "encoder.5": s1_64,
        "encoder.8": (L2, (64, 128, 2, 1, C5, L4), (128, 64, 1, 2, ops.UP2, L2), (64, 128, 2, 1, W5, L4, (5, 320, 1))),
        "encoder.11": s1_128,
        T + "0": (L4, (128, 128, 1, 1, ops.taps_conv(5, 1, 0), La), (128, 128, 1, 1, ops.taps_conv_dgrad_s1(5, 1, 0), L4),
                  (128, 128, 1, 1, [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)], La, (5, 640, 1))),
        T + "3": (La, (128, 128, 1, 1, ops.taps_conv(3, 2, 0), Lb), (128, 128, 1, 1, ops.taps_conv_dgrad_s1(3, 2, 0), La),
                  (128, 128, 1, 1, [(0, 0), (2, 0), (4, 0)], Lb, (3, 384, 1))),
        T + "6": (Lb, (128, 128, 1, 1, ops.taps_conv(3, 3, 0), Lc), (128, 128, 1, 1, ops.taps_conv_dgrad_s1(3, 3, 0), Lb),
                  (128, 128, 1, 1, [(0, 0), (3, 0), (6, 0)], Lc, (3, 384, 1))),
        "decoder.0": s1_128,
        "decoder.1": (L4, (128, 64, 1, 2, ops.UP2, L2), (64, 128, 2, 1, ops.taps_convT_dgrad(), L4),
                      (128, 64, 1, 2, WT, L4, (320, 5, 1))),
        "decoder.4": s1_64,
        "decoder.5": (L2, (64, 32, 1, 2, ops.UP2, Ltot), (32, 64, 2, 1, ops.taps_convT_dgrad(), L2),
                      (64, 32, 1, 2, WT, L2, (160, 5, 1))),
    }


def check(layers, tables):
    assert list(layers) == list(tables)
    for name, (Lin, fwd, dgrad, wgrad) in tables.items():
        g = layers[name]
        assert (g.key, g.bias) == (name + ".weight", name + ".bias")
        assert g.fwd(Lin) == fwd, name
        assert g.dgrad(Lin) == dgrad, name
        assert g.wgrad(Lin) == wgrad, name
        assert g.lout(Lin) == fwd[5] and g.lin(fwd[5]) == Lin, name


@pytest.mark.parametrize("Ltot", [960, 1040])                               # T = 12, 13
def test_convae_launch_geometry(lay, Ltot):
    check(lay[0], convae_tables(Ltot))


@pytest.mark.parametrize("Ltot", [960, 1040])
def test_convreconstruction_launch_geometry(lay, Ltot):
    ae = convae_tables(Ltot)
    check(lay[1], {"encoder.3": ae["encoder.2"], "encoder.6": ae["encoder.5"], "encoder.9": ae["decoder.5"]})


def test_pack_plan():
    """the 22 (weight, use) pairs the step packed, in the order of the hand-kept list, and their pack geometry"""
    conv = ["encoder.2", "encoder.5", "encoder.8", "encoder.11", T + "0", T + "3", T + "6", "decoder.0", "decoder.4"]
    convT = ["decoder.1", "decoder.5"]
    want = ([(k + ".weight", "conv_fwd") for k in conv] + [(k + ".weight", "convT_fwd") for k in convT]
            + [(k + ".weight", "conv_dgrad") for k in conv] + [(k + ".weight", "convT_dgrad") for k in convT])
    model = ConvAutoencoder()
    assert model.pack_plan == want and len(set(want)) == 22
    shapes = {k: tuple(p.shape) for k, p in model.named_parameters()}
    geo = {(k, kind): ops._pack_geometry(shapes[k], kind) for k, kind in model.pack_plan}
    assert geo["encoder.2.weight", "conv_fwd"] == (5, 32, 64, 5, 160)
    assert geo["encoder.2.weight", "conv_dgrad"] == (5, 64, 32, 160, 5)
    assert geo["encoder.8.weight", "conv_fwd"] == (5, 64, 128, 5, 320)
    assert geo["encoder.8.weight", "conv_dgrad"] == (5, 128, 64, 320, 5)
    assert geo[T + "3.weight", "conv_fwd"] == (3, 128, 128, 3, 384)
    assert geo[T + "3.weight", "conv_dgrad"] == (3, 128, 128, 384, 3)
    assert geo["decoder.1.weight", "convT_fwd"] == (5, 128, 64, 320, 5)
    assert geo["decoder.1.weight", "convT_dgrad"] == (5, 64, 128, 5, 320)
    assert geo["decoder.5.weight", "convT_fwd"] == (5, 64, 32, 160, 5)
    assert geo["decoder.5.weight", "convT_dgrad"] == (5, 32, 64, 5, 160)
    for k in ("encoder.11", T + "0", "decoder.0"):
        assert geo[k + ".weight", "conv_fwd"] == (5, 128, 128, 5, 640)
        assert geo[k + ".weight", "conv_dgrad"] == (5, 128, 128, 640, 5)
    for k in ("encoder.5", "decoder.4"):
        assert geo[k + ".weight", "conv_fwd"] == (5, 64, 64, 5, 320)
        assert geo[k + ".weight", "conv_dgrad"] == (5, 64, 64, 320, 5)
    assert geo[T + "6.weight", "conv_fwd"] == geo[T + "3.weight", "conv_fwd"]
    assert geo[T + "6.weight", "conv_dgrad"] == geo[T + "3.weight", "conv_dgrad"]


@pytest.mark.parametrize("mod", [nn.Conv1d(8, 8, 3, stride=2, padding=1), nn.ConvTranspose1d(8, 8, 4, 2, 1),
                                 nn.ConvTranspose1d(8, 8, 5, 2, 2)], ids=["conv_k3s2", "convT_k4", "convT_op0"])
def test_untested_geometry_is_refused(mod):
    with pytest.raises(SaHipError):
        ops.ConvGeom.of("layer", mod)
