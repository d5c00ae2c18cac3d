"""The paths whose programs hold the nine op kinds of ABI 8 -- editing, inversion, composed guidance, DPM-Solver++, the diffusion objective,
the MS-VQGAN reconstruction -- bit for bit against what tests/golden/record_opkind_bits.py recorded on an MI355X from the last commit on
which those launches were side launchers next to the executor (tests/golden/opkind_bits.npz).  The change is host code over unchanged
kernels: the same launches in the same order give the same bits, so the comparison is np.array_equal.  The patch-wise loops and
DPM-Solver++ under classifier-free guidance are pinned by tests/test_engine_bits_gpu.py (patch_ddim, patch_plms, dpm2_logsnr_cfg)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import golden  # noqa: E402
import record_opkind_bits as rec  # noqa: E402


@pytest.mark.parametrize("group", rec.GROUPS)
def test_opkind_bits_are_those_of_the_side_launchers(group, monkeypatch):
    """Static GEMM tiles on both sides (the tile cache has no say) and GRAPH_STEPS = 4, so the K-step bodies are replayed."""
    from frido_amd import runtime, tune
    monkeypatch.setattr(tune, "ENABLED", False)
    monkeypatch.setattr(runtime, "GRAPH_STEPS", 4)
    g = golden("opkind_bits")
    got = rec.runs(group)
    runs = sorted(k for k in got if "." not in k)
    assert runs and sorted(got) == sorted(k for k in g.files if k.split(".")[0] in runs)
    for k in sorted(got):
        same = np.array_equal(got[k], g[k])
        if "." not in k:
            print(f"{k}: {'identical' if same else 'max-abs difference %.3e' % float(np.abs(got[k] - g[k]).max())}")
        assert same, k


def test_opkind_bits_fixture_covers_every_group_and_tells_the_options_apart():
    g = golden("opkind_bits")
    runs = {k for k in g.files if "." not in k}
    assert {"edit_philox", "edit_tape", "invert_cfg", "compose_ddim", "compose_dpm", "dpm2_plain", "loss_philox", "loss_tape", "msvq_plain",
            "msvq_aux"} == runs
    assert all(np.isfinite(g[k]).all() for k in g.files)
    for a, b in rec.DIFFERENT:
        assert not np.array_equal(g[a], g[b]), (a, b)
