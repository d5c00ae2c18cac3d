"""The Python front end over the HIP programs -- the first-stage classes and DecoderRuntime's plan getters, the patch-wise decode / encode
and the plans they share with the whole-latent calls, the two text towers and their plan LRU, the objective on LossEngine (stream
hand-over, graph LRU, the host draws), PyUNetModel.forward and the runtime swaps of ema_scope -- bit for bit against what
tests/golden/record_frontend_bits.py recorded on an MI355X from the commit before that plumbing was folded
(tests/golden/frontend_bits.npz).  It is host code over unchanged kernels: the same launches in the same order on the same streams give
the same bits, so the comparison is np.array_equal."""
import numpy as np
import pytest

from helpers import golden
import record_frontend_bits as rec


@pytest.mark.gpu
@pytest.mark.parametrize("group", rec.GROUPS)
def test_frontend_bits_are_those_of_the_front_end_before_the_refactor(group, monkeypatch):
    """Static GEMM tiles on both sides: the tile cache has no say."""
    from frido_amd import tune
    monkeypatch.setattr(tune, "ENABLED", False)
    g = golden("frontend_bits")
    got = rec.runs(group)
    assert sorted(got) == sorted(k for k in g.files if k.startswith(group + "."))
    for k in sorted(got):
        same = got[k].dtype == g[k].dtype and np.array_equal(got[k], g[k])
        print(f"{k}: {'identical' if same else 'DIFFERENT'}")
        assert same, k


def test_frontend_bits_fixture_covers_every_group_and_tells_the_options_apart():
    g = golden("frontend_bits")
    assert all(any(k.startswith(group + ".") for k in g.files) for group in rec.GROUPS)
    assert {"first_stage.dec_forced", "msvq.fwd_aux.2", "msvq.log", "patch.whole_dec.whole_first", "patch.enc", "cond.bert.a_rebuilt",
            "cond.clip.encode", "objective.forward.torch", "objective.mix9", "denoiser.ema_in2"} <= set(g.files)
    # (entries stored as SHA-256 digests are uint8: the recorder checked their tensors to be finite before it hashed them)
    assert all(np.isfinite(g[k]).all() for k in g.files)
    for a, b in rec.DIFFERENT:
        assert a in g.files and b in g.files and not np.array_equal(g[a], g[b]), (a, b)
    # what ran twice -- a replayed graph, a rebuilt plan, a plan first built by the other caller, a runtime put back -- gave the same bits
    # ("np" and "pil" too: the two conversions are the same real product rounded once, see record_frontend_bits.DIFFERENT)
    for a, b in (("first_stage.dec_np", "first_stage.dec_pil"), ("msvq.fwd.1", "msvq.fwd.2"), ("msvq.fwd_aux.1", "msvq.fwd_aux.2"), ("first_stage.dec", "first_stage.dec_again"),
                 ("cond.bert.a", "cond.bert.a_rebuilt"), ("patch.dec", "patch.dec.whole_first"), ("patch.enc", "patch.enc.whole_first"),
                 ("patch.whole_dec", "patch.whole_dec.whole_first"), ("objective.mix0", "objective.mix9"),
                 ("denoiser.s1", "denoiser.after"), ("denoiser.ema_in", "denoiser.ema_in2"), ("denoiser.ema_in", "denoiser.ema_plain")):
        assert np.array_equal(g[a], g[b]), (a, b)
