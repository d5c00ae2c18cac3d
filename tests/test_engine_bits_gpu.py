"""Every path through runtime.SamplerEngine -- the four kinds, host and Philox noise, K-step units, callbacks, noise dropout, the eager
score-corrector loops, patch mode, class labels, guidance -- bit for bit against what tests/golden/record_engine_bits.py recorded on an
MI355X from the commit before the engine got one step-body builder and one replay loop (tests/golden/sampler_engine_bits.npz).  The
engine is host code over unchanged kernels: the same ops in the same order give the same bits, so the comparison is np.array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
import record_engine_bits as rec  # noqa: E402


@pytest.mark.parametrize("group", rec.GROUPS)
def test_engine_bits_are_those_of_the_engine_before_the_refactor(group, monkeypatch):
    """Static GEMM tiles on both sides (the tile cache has no say) and GRAPH_STEPS = 4, so the 10-step stages replay as [1, 4, 4, 1]."""
    from frido_amd import runtime, tune
    monkeypatch.setattr(tune, "ENABLED", False)
    monkeypatch.setattr(runtime, "GRAPH_STEPS", 4)
    g = golden("sampler_engine_bits")
    got = rec.runs(group)
    runs = sorted(k for k in got if "." not in k)
    assert runs and sorted(got) == sorted(k for k in g.files if k.split(".")[0] in runs)
    for k in sorted(got):
        same = np.array_equal(got[k], g[k])
        if "." not in k:
            print(f"{k}: {'identical' if same else 'max-abs difference %.3e' % float(np.abs(got[k] - g[k]).max())}")
        assert same, k


def test_engine_bits_fixture_covers_every_kind_and_tells_the_options_apart():
    g = golden("sampler_engine_bits")
    runs = {k for k in g.files if "." not in k}
    assert {"ddim_tape", "plms_tape_cfg", "dpm2_logsnr_cfg", "anc_loop_tape", "patch_ddim", "labels_ddim_cfg"} <= runs
    assert all(np.isfinite(g[k]).all() for k in g.files)
    for a, b in rec.DIFFERENT:
        assert a in runs and b in runs and not np.array_equal(g[a], g[b]), (a, b)
