"""The form of a training step without a GPU: HipEncoderEngine._decide_step on plain plan dicts, against the library's real
host-side *_supported queries.  One function decides, before the first launch, which convolution form every block runs, which blocks
leave pool extremes / pairs / centred tiles, which BatchNorm-backward sums come out of a dgrad GEMM and whether the step's tail is one
launch; _forward_range, the heads and backward() only read what it wrote.  So the launches a configuration produces at cfg-A's real
size -- 128 pairs of 12000-sample windows, far past what a test can run -- are checked here, where nothing is launched.  That the
launch sequence itself follows these keys: tools/step_trace.py, tests/test_gpu_fold.py, tests/test_gpu_e2e.py."""
import pytest

from voicemap_amd import _lib
from voicemap_amd.engine import HEADS, HipEncoderEngine, _DT

FORM = ("e_now", "pairs_now", "ctr_now", "bnred_now")


def _engine(f, dtype, **switches):
    blocks = [(32, f, 4), (3, 2 * f, 2), (3, 3 * f, 2), (3, 4 * f, 2)]

    class FormOnly(HipEncoderEngine):                          # no GPU: an engine that is only what _decide_step reads
        def __init__(self):
            self.lib, self.blocks, self.nb, self.E, self.dtype = _lib.lib(), blocks, len(blocks), 64, _DT[dtype]
            self.head = "uniform_euclidean"
            is16 = self.is16 = dtype in ("f16", "bf16")
            self.fuse_block1 = is16                            # the defaults of HipEncoderEngine.__init__
            self.wt = {i: None for i in range(1, len(blocks))} if is16 else {}
            self.pooled_reduce = self.fused_bn_reduce = self.fold_affine = self.fused_infer_pool = is16
            self.fused_sums_finalize = self.fold_pairs = self.split_towers = self.fused_tail = True
            self.fused_pool_extreme = self.sync_bn = False
            self.center_blocks = (1,)
            for k, v in switches.items():
                assert hasattr(self, k), k
                setattr(self, k, v)
    return FormOnly()


def _decide(eng, pairs, l0=12000, masks=False, defer_tail=True):
    ls = [l0]
    for (_, _, p) in eng.blocks:
        ls.append(ls[-1] // p)
    pl = {"n": 2 * pairs, "L": ls, "training": True, **{i: {} for i in range(eng.nb)}}
    eng._decide_step(pl, pairs, [object()] * eng.nb if masks else None, defer_tail)
    return pl, {k: tuple(bool(pl[i][k]) for i in range(eng.nb)) for k in FORM}, tuple(pl[i]["conv"] for i in range(eng.nb))


def test_every_entry_of_the_form_is_written_on_every_call():
    eng = _engine(128, "f16")
    pl, _, _ = _decide(eng, 128)
    eng.fold_affine = eng.fused_bn_reduce = eng.fused_tail = False   # a second decision on the same plan leaves nothing of the first
    pl2, form, conv = _decide(eng, 128)
    assert set(pl2) == set(pl) and all(set(pl2[i]) == {"conv", *FORM} for i in range(4))
    assert not pl2["fold_now"] and not pl2["tail_pending"] and not pl2["tail_parts"]
    assert not any(any(v) for v in form.values()) and conv == ("fused1", "plain", "plain", "plain")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_cfg_a_at_real_size(dtype):
    pl, form, conv = _decide(_engine(128, dtype), 128)
    assert pl["fold_now"] is True and conv == ("fused1", "fold", "fold", "fold")
    assert form["e_now"] == form["pairs_now"] == (False, True, True, False)
    assert form["ctr_now"] == (False, dtype == "f16", False, False)
    assert form["bnred_now"] == (True, True, True, False)
    assert pl["tail_pending"] is True and pl["tail_parts"] is True


def test_cfg_a_switches_that_leave_the_fold_on():
    _, form, _ = _decide(_engine(128, "f16", center_blocks=()), 128)
    assert form["ctr_now"] == (False,) * 4 and form["pairs_now"] == (False, True, True, False)
    pl, form, conv = _decide(_engine(128, "f16", fold_pairs=False), 128)
    assert pl["fold_now"] and conv[1:] == ("fold",) * 3 and form["e_now"] == (False, True, True, False)
    assert form["pairs_now"] == form["ctr_now"] == (False,) * 4       # only a pair-form tile is centred


def test_cfg_a_with_dropout_masks():
    pl, form, conv = _decide(_engine(128, "f16"), 128, masks=True)
    assert pl["fold_now"] is False and conv == ("fused1", "plain", "plain", "plain")
    assert form["e_now"] == form["pairs_now"] == form["ctr_now"] == (False,) * 4
    assert form["bnred_now"] == (True, True, True, False)
    assert pl["tail_pending"] and pl["tail_parts"]


def test_the_mixed_case_baseline_64():
    """32 pairs of 12000: the fold is refused at block 3 and vm_conv_dgrad_bnred serves block 3's dgrad only."""
    lib, n, dt = _lib.lib(), 64, _DT["f16"]
    geo = [(3000, 64, 128), (1500, 128, 192), (750, 192, 256)]
    assert [lib.query("vm_conv_fwd_fold_supported", n, *g, dt, int(j < 2)) for j, g in enumerate(geo)] == [1, 0, 1]
    assert [lib.query("vm_conv_dgrad_bnred_supported", n, *g, dt) for g in geo] == [0, 1, 0]
    pl, form, conv = _decide(_engine(64, "f16"), 32)
    assert pl["fold_now"] is False and conv == ("fused1", "plain", "plain", "plain")
    assert form["bnred_now"] == (False, True, False, False) and form["e_now"] == (False,) * 4
    pl, form, conv = _decide(_engine(64, "f16", fused_pool_extreme=True), 32)
    assert form["e_now"] == (False, True, False, False) and conv == ("fused1", "e", "plain", "plain")
    assert form["bnred_now"] == (False, True, False, False) and form["pairs_now"] == (False,) * 4


def test_f32_fuses_nothing_but_the_tail():
    pl, form, conv = _decide(_engine(128, "f32"), 128)
    assert pl["fold_now"] is False and conv == ("plain",) * 4 and not any(any(v) for v in form.values())
    assert pl["tail_pending"] is True and pl["tail_parts"] is True       # follows fused_tail and vm_tail_fwd_bwd_supported alone
    pl, _, _ = _decide(_engine(128, "f32", fused_tail=False), 128)
    assert pl["tail_pending"] is False and pl["tail_parts"] is False


def test_when_the_tail_is_not_deferred():
    pl, form, _ = _decide(_engine(128, "f16"), 128, defer_tail=False)
    assert pl["tail_pending"] is False and pl["tail_parts"] is False and pl["fold_now"] is True
    assert form["bnred_now"] == (True, True, True, False)
    assert _lib.lib().query("vm_tail_fwd_bwd_supported", 512, 64) == 1 and _lib.lib().query("vm_tail_fwd_bwd_supported", 2048, 64) == 0
    pl, _, _ = _decide(_engine(512, "f16"), 4, l0=4064)                  # a last block of 2048 channels: vm_tail_fwd_bwd refuses it
    assert pl["tail_pending"] is False and pl["tail_parts"] is False
    eng = _engine(128, "f16", head="classifier")                         # not a siamese head
    assert eng.head not in HEADS and _decide(eng, 128)[0]["tail_pending"] is False


def test_range_sized_queries_take_the_windows_a_range_gets():
    """vm_conv_fwd_e is launched per tower when the towers are split: its query is asked at that size."""
    asked = []

    class Spy:
        def __init__(self, lib):
            self.lib = lib

        def query(self, name, *a):
            asked.append((name, a[0]))
            return self.lib.query(name, *a)
    for split, want in ((True, 32), (False, 64)):
        eng = _engine(64, "f16", fused_pool_extreme=True, split_towers=split)
        eng.lib = Spy(eng.lib)
        del asked[:]
        _decide(eng, 32)
        assert {n for name, n in asked if name == "vm_conv_fwd_e_supported"} == {want}
        assert {n for name, n in asked if name == "vm_conv_dgrad_bnred_supported"} == {64}
        names = [name for name, _ in asked]
        assert names.count("vm_conv_dgrad_bnred_supported") == 3 and names.count("vm_tail_fwd_bwd_supported") == 1   # each once
