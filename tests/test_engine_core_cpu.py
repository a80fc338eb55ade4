"""The shared core of the two engines without a GPU (voicemap_amd/engine_core.py): the flat layout both engines adopt, the initial
draw, the surface bench.py drives, and the capability attributes models.py / utils.py ask instead of probing.  The layout literals and
the two digests were taken from the constructors' arithmetic before the core existed: a given seed keeps giving the same bits."""
import hashlib

import numpy as np
import pytest

from voicemap_amd.engine import FlatState, HipEncoderEngine, flat_layout
from voicemap_amd.engine_core import EngineCore, initial_params, require_resident_input
from voicemap_amd.spectro_engine import HipSpectrogramEncoderEngine, band_stacked_spec, stack_bands, unstack_bands

# (filters, E, head) -> (conv kernels' stored shapes, offsets of every tensor in spec order, n_flat, moving-statistics offsets, NT size)
LAYOUT_2D = {
    (8, 16, "weighted_l1"): ([(3, 8, 8), (3, 24, 16), (3, 48, 24), (3, 72, 32)],
                             [0, 192, 256, 320, 384, 1536, 1600, 1664, 1728, 5184, 5248, 5312, 5376, 12288, 12352, 12416, 12480, 12992,
                              13056, 13120], 13184, [0, 64, 128, 192, 256, 320, 384, 448], 512),
    (32, 64, "uniform_euclidean"): ([(3, 8, 32), (3, 96, 64), (3, 192, 96), (3, 288, 128)],
                                    [0, 768, 832, 896, 960, 19392, 19456, 19520, 19584, 74880, 75008, 75136, 75264, 185856, 185984,
                                     186112, 186240, 194432, 194496, 194560], 194624, [0, 64, 128, 192, 256, 384, 512, 640], 768),
}


@pytest.mark.parametrize("cfg", sorted(LAYOUT_2D))
def test_the_2d_store_is_laid_out_as_its_constructor_used_to(cfg):
    kernels, offs, n_flat, nt, n_nt = LAYOUT_2D[cfg]
    spec, chan, cin, cs = band_stacked_spec(*cfg)
    st = FlatState.from_spec(spec, chan, "cpu")
    head = {"weighted_l1": (cfg[1], 1), "uniform_euclidean": (1, 1)}[cfg[2]]
    names = [f"{l}{i}.{t}" for i in range(1, 5) for l, t in (("conv", "kernel"), ("conv", "bias"), ("bn", "gamma"), ("bn", "beta"))]
    names += ["dense.kernel", "dense.bias", "head.kernel", "head.bias"]
    shapes = [s for k, c in zip(kernels, chan) for s in (k, (c,), (c,), (c,))] + [(chan[-1], cfg[1]), (cfg[1],), head, (1,)]
    assert list(st.offsets) == names
    assert [v[0] for v in st.offsets.values()] == offs and [v[2] for v in st.offsets.values()] == shapes
    assert all(v[1] == int(np.prod(v[2])) for v in st.offsets.values())
    assert st.n_flat == n_flat == st.P.numel() == st.G.numel() == st.M.numel() == st.V.numel()
    assert list(st.nt_off) == [f"bn{i}.moving_{s}" for i in range(1, 5) for s in ("mean", "variance")]
    assert [v[0] for v in st.nt_off.values()] == nt and [v[1] for v in st.nt_off.values()] == [c for c in chan for _ in range(2)]
    assert st.NT.numel() == n_nt
    assert cin == [1] + chan[:-1] and cs == [k[1] for k in kernels]


@pytest.mark.parametrize("blocks,head,classes", [([(32, 8, 4), (3, 16, 2)], "uniform_euclidean", 0),
                                                 ([(32, 16, 4), (3, 32, 2), (3, 48, 2), (3, 64, 2)], "classifier", 7)])
def test_the_1d_constructor_form_is_flat_layout(blocks, head, classes):
    spec, offsets, n_flat, nt_off, n_nt = flat_layout(blocks, 16, head, classes)
    st = FlatState(blocks, 16, head, classes, "cpu")
    assert st.spec == spec and st.offsets == offsets and list(st.offsets) == list(offsets) and st.n_flat == n_flat
    assert st.nt_off == nt_off and st.NT.numel() == n_nt and st.n_params == sum(n for _, n, _ in offsets.values())
    again = FlatState.from_spec(spec, [c for _, c, _ in blocks], "cpu")
    assert again.offsets == offsets and again.nt_off == nt_off and again.n_flat == n_flat


def _digest(offsets, params, to_stored=lambda name, a: a):
    """sha256 over the fp32 tensors in layout order, each in its stored form."""
    h = hashlib.sha256()
    for name, (_, n, shape) in offsets.items():
        a = to_stored(name, np.asarray(params[name], dtype=np.float32))
        assert a.shape == tuple(shape) and a.size == n
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_the_initial_draw_of_a_seed_keeps_its_bits():
    st = FlatState([(32, 8, 4), (3, 16, 2)], 16, "uniform_euclidean", 0, "cpu")
    p = initial_params(st.offsets, 1234)
    assert _digest(st.offsets, p) == "4d70c6253ec0d801b2bf494ee1ef604fdae8fce178dfaa3ef4fef7f5247107f1"
    assert float(p["bn2.gamma"].min()) == 1.0 and not p["conv1.bias"].any() and not p["bn1.beta"].any()
    spec, chan, cin, cs = band_stacked_spec(8, 16, "weighted_l1")
    st = FlatState.from_spec(spec, chan, "cpu")

    class HooksOnly(HipSpectrogramEncoderEngine):              # no GPU: an engine that is only its public <-> stored hooks
        def __init__(self):
            self.offsets, self.chan, self.cin, self.cs = st.offsets, chan, cin, cs
    eng = HooksOnly()
    p = initial_params(st.offsets, 1234, eng.public_shape)
    assert p["conv3.kernel"].shape == (3, 3, 16, 24) and eng.public_shape("dense.kernel") == (32, 16)
    assert _digest(st.offsets, p, eng._to_stored) == "661354f14174a7d575fa616646c39af00e7c5af7e41f7e641381ae5fd72f067a"
    back = eng._to_public("conv3.kernel", eng._to_stored("conv3.kernel", p["conv3.kernel"].astype(np.float32)))
    assert np.array_equal(back, p["conv3.kernel"].astype(np.float32)) and eng._to_public("bn1.gamma", p["bn1.gamma"]) is p["bn1.gamma"]
    k1 = stack_bands(p["conv1.kernel"].astype(np.float32), cs[0])          # block 1: three real rows of eight, the rest zero padding
    assert k1.shape == (3, 8, 8) and not k1[:, 3:].any() and np.array_equal(unstack_bands(k1, 1), p["conv1.kernel"].astype(np.float32))
    assert stack_bands(k1, cs[0]) is k1                                    # a kernel already in its stored form is taken as it is


def test_both_engines_have_what_bench_drives_and_the_core_has_no_architecture():
    for name in ("refresh_weights", "adjust_loss_scale", "skipped_steps", "get_params", "plan", "preprocess", "forward", "siamese_head",
                 "backward", "optimizer_step", "_call"):
        assert callable(getattr(HipEncoderEngine, name)), name
    for name in ("plan", "features", "forward", "siamese_head", "backward", "optimizer_step", "get_params", "_call"):
        assert callable(getattr(HipSpectrogramEncoderEngine, name)), name
    core_sets = set(EngineCore.__init__.__code__.co_names) | set(EngineCore._init_zero_debias.__code__.co_names)
    assert {"P", "M", "V", "NT", "ZD", "bn_steps", "iterations", "n_flat", "lib", "timed", "overlap_wgrad", "grad_sync"} <= core_sets
    assert {"split_towers", "pre_overlap"} <= set(HipEncoderEngine.__init__.__code__.co_names)
    for name in ("plan", "forward", "backward", "refresh_weights"):
        assert name not in vars(EngineCore), name
    assert issubclass(HipEncoderEngine, EngineCore) and issubclass(HipSpectrogramEncoderEngine, EngineCore)
    assert not issubclass(HipSpectrogramEncoderEngine, HipEncoderEngine)
    assert HipEncoderEngine.losses == {"siamese", "classifier", "prototypical", "triplet", "margin"} and HipEncoderEngine.resident_input
    assert HipSpectrogramEncoderEngine.losses == {"siamese"} and not HipSpectrogramEncoderEngine.resident_input


def test_the_resident_input_guard_asks_the_class():
    class Raw:
        resident_input = False

    class Resident:
        resident_input = True
    require_resident_input(Resident)
    with pytest.raises(NotImplementedError, match="the spectrogram engine takes raw windows; its front-end is vm_stft_logmel"):
        require_resident_input(Raw)
    require_resident_input(HipEncoderEngine)
    with pytest.raises(NotImplementedError):
        require_resident_input(HipSpectrogramEncoderEngine)
