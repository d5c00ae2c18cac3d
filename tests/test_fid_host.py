"""Host side of the Fréchet Inception Distance (frido_amd/fid.py, models.FIDInceptionV3, pipeline.fid*): the tables, the folding, the
float64 restatement's own properties, the statistics, the distance, the refusals and the ABI constraints.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from frido_amd import _lib, synth
from frido_amd._lib import FridoHipError

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def net():
    from frido_amd.models import FIDInceptionV3
    m = FIDInceptionV3()
    sd = R.fill(m)
    return m, sd


def _images(tag, B, s):
    return torch.from_numpy(synth.seeded_normal(tag, (B, 3, s, s))).clamp(-1, 1)


# ---- the network's shape ----------------------------------------------------------------------------------
def test_state_dict_keys_and_parameter_count(net):
    from frido_amd import fid
    m, _ = net
    table = fid.conv_table()
    assert len(table) == 94 and len({r[0] for r in table}) == 94
    want = {"fc.weight", "fc.bias"}
    for name, *_ in table:
        want |= {f"{name}.conv.weight"} | {f"{name}.bn.{k}" for k in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(m.state_dict()) == want
    assert {"Conv2d_1a_3x3.conv.weight", "Mixed_5b.branch1x1.bn.running_var", "Mixed_7c.branch_pool.conv.weight",
            "Mixed_7b.branch3x3dbl_3b.bn.bias", "Mixed_6e.branch7x7dbl_5.conv.weight"} <= want
    n_conv_bn = sum(p.numel() for k, p in m.named_parameters() if not k.startswith("fc."))
    assert n_conv_bn == 21_785_568
    assert n_conv_bn + 1000 * 2048 + 1000 == 23_834_568                      # with torchvision's 1000-class fc: its published count
    assert tuple(m.fc.weight.shape) == (1008, 2048) and tuple(m.fc.bias.shape) == (1008,)      # the FID checkpoint's fc, held, never run
    assert not any(p.requires_grad for p in m.parameters()) and not m.training
    assert m.Mixed_6b.branch7x7_2.conv.kernel_size == (1, 7) and m.Mixed_6b.branch7x7_2.conv.padding == (0, 3)
    assert m.Mixed_7b.branch3x3_2b.conv.kernel_size == (3, 1) and m.Mixed_7b.branch3x3_2b.conv.padding == (1, 0)
    assert m.Conv2d_1a_3x3.bn.eps == 1e-3 and m.Conv2d_1a_3x3.conv.bias is None
    geoms = {(r[3], r[4], r[5], r[6], r[7]) for r in table}                 # (kh, kw, stride, pad, padx)
    assert {(3, 3, 2, 0, 0), (5, 5, 1, 2, 2), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0), (3, 3, 1, 0, 0)} <= geoms
    assert fid.tower_planes(299) == dict(Mixed_5b=35, Mixed_5c=35, Mixed_5d=35, Mixed_6a=35, Mixed_6b=17, Mixed_6c=17, Mixed_6d=17,
                                         Mixed_6e=17, Mixed_7a=17, Mixed_7b=8, Mixed_7c=8, head=8)
    assert fid.tower_planes(107)["Mixed_5b"] == 11 and fid.tower_planes(107)["Mixed_6b"] == 5 and fid.tower_planes(107)["head"] == 2
    assert [sum(fid.block_widths(n)) for n in fid.BLOCKS] == [256, 288, 288, 768, 768, 768, 768, 768, 1280, 2048, 2048]
    assert tuple(fid.BLOCKS) == R.BLOCK_NAMES


def test_the_table_and_the_restatement_name_the_same_convs(net):
    """Every conv of the table is run by the restatement with the table's geometry (the recorded outputs' shapes follow from it)."""
    from frido_amd import fid
    _, sd = net
    rec, inputs = {}, {}
    R.Net(sd, torch.float64, True, rec).tower(R.preprocess(R.to_q(_images("fid:host107", 1, 107)), 107), inputs)
    table = fid.conv_table()
    assert set(rec) == {r[0] for r in table}
    assert [r[0] for r in table] == list(rec)                                # the same order, too
    for name, cin, cout, *_ in table:
        assert rec[name].shape[1] == cout and sd[name + ".conv.weight"].shape[:2] == (cout, cin)
    for n, (kind, cin, _) in fid.BLOCKS.items():
        assert inputs[n].shape[1] == cin and inputs[n].shape[2] == fid.tower_planes(107)[n]


def test_filler_keeps_every_layer_alive_and_in_range(net):
    """Section 5 of the issue: running variances positive; in the float64 reference at the test inputs every one of the 94 post-ReLU
    outputs has >= 20 % non-zero entries and a largest magnitude in [1e-2, 1e2] (measured when written: >= 40 %, 5.3 .. 40)."""
    _, sd = net
    assert all(float(v.min()) > 0 for k, v in sd.items() if k.endswith("running_var"))
    for tag, B, s in (("fid:img107", 2, 107), ("fid:img299", 1, 299)):
        rec = {}
        R.Net(sd, torch.float64, True, rec).tower(R.preprocess(R.to_q(_images(tag, B, s)), s))
        assert len(rec) == 94
        for name, v in rec.items():
            assert float((v > 0).double().mean()) >= 0.20, (s, name)
            assert 1e-2 <= float(v.max()) <= 1e2, (s, name, float(v.max()))
    with pytest.raises(ValueError):
        synth.fill_tensor("x.weight", (4, 4), "no-such-profile")


def test_batchnorm_folding_against_the_unfolded_net(net):
    """a = gamma / sqrt(var + 1e-3), w' = w a, b' = beta - mean a in float64, rounded once: per conv exactly the float32 rounding of the
    float64 fold, and the folded float64 tower within the rounding of its 94 weight tensors of the unfolded one."""
    from frido_amd import fid
    _, sd = net
    w = fid.folded_weights(sd, "cpu")
    assert len(w) == 188
    for name in ("Conv2d_1a_3x3", "Mixed_6c.branch7x7dbl_3", "Mixed_7c.branch3x3_2b"):
        a = sd[name + ".bn.weight"].double() / torch.sqrt(sd[name + ".bn.running_var"].double() + 1e-3)
        assert torch.equal(w[name + ".weight"], (sd[name + ".conv.weight"].double() * a.view(-1, 1, 1, 1)).float())
        assert torch.equal(w[name + ".bias"], (sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * a).float())
        assert w[name + ".weight"].dtype == torch.float32
    x = R.preprocess(R.to_q(_images("fid:img107", 2, 107)), 107)
    f_fold = R.Net(sd, torch.float64, True).tower(x)
    f_raw = R.Net(sd, torch.float64, False).tower(x)
    err = float((f_fold - f_raw).abs().max() / f_raw.abs().max())
    print(f"folded vs unfolded float64 tower: {err:.2e} relative")
    assert 0 < err < 94 * 2.0 ** -24                                          # each layer's weights and bias are rounded to float32 once


# ---- the formulas of the restatement ----------------------------------------------------------------------
def test_average_pool_is_count_exclude_pad():
    for shape in ((2, 4, 7, 7), (1, 8, 5, 6), (1, 4, 2, 2), (1, 4, 1, 3)):
        x = torch.from_numpy(synth.seeded_normal(f"fid:pool{shape}", shape)).double()
        ours = R.avg_pool_in_order(x)
        ref = F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)
        assert float((ours - ref).abs().max()) <= 4 * 2.0 ** -53 * float(x.abs().max()) * 9
        if min(shape[2:]) >= 2:
            wrong = F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=True)
            assert float((ours - wrong).abs()[:, :, 0, 0].min()) > 1e-6      # the corner divides by 4, not 9


def test_identity_resize_and_both_quantisers():
    q = torch.randint(0, 256, (2, 3, 16, 16), generator=torch.Generator().manual_seed(3)).float()
    for dtype in (torch.float32, torch.float64):
        out = R.preprocess(q, 16, dtype)
        assert torch.equal(out, ((q.to(dtype) - 128) / 128))                # S x S comes back exactly
    # the quantisers, against the script's own expressions (numpy's astype(uint8) and torch's .to(uint8) truncate)
    x = torch.cat([torch.linspace(-1.2, 1.2, 4001), torch.tensor([(2 * k + 1) / 255.0 - 1 for k in range(255)])]).float()
    pil = (255 * ((torch.clamp(x, -1., 1.) + 1.) / 2.).numpy()).astype(np.uint8)              # custom_to_pil
    npy = ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8).numpy()                             # custom_to_np
    assert np.array_equal(R.quantise(x, "pil").numpy().astype(np.uint8), pil)
    assert np.array_equal(R.quantise(x, "np").numpy().astype(np.uint8), npy)
    # (the two are the same function of a real number and differ in the order of their roundings only: no input among 4 million
    #  random ones and the 254 level boundaries separates them, so nothing here can assert that they differ)
    img = x[:3 * 32 * 32].view(1, 3, 32, 32)
    assert torch.equal(R.to_q(img, "pil"), torch.from_numpy(pil[:3072].astype(np.float64)).view(1, 3, 32, 32))
    u8 = torch.from_numpy(pil[:3072]).view(1, 3, 32, 32).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(R.to_q(u8), R.to_q(img, "pil"))                       # the uint8 layout of the same image
    # the resize: a 2 x 2 image to 4 x 4 by hand (scale 0.5: sources 0, 0.5, 1, 1.5 -> the last clamps its right neighbour)
    q2 = torch.tensor([[0.0, 100.0], [200.0, 40.0]]).view(1, 1, 2, 2).expand(1, 3, 2, 2)
    got = R.preprocess(q2, 4)[0, 0] * 128 + 128
    want = torch.tensor([[0, 50, 100, 100], [100, 85, 70, 70], [200, 120, 40, 40], [200, 120, 40, 40]], dtype=torch.float64)
    assert torch.equal(got, want)


# ---- checkpoint, refusals ---------------------------------------------------------------------------------
def test_checkpoint_round_trip_also_without_num_batches_tracked(net, tmp_path):
    from frido_amd.models import FIDInceptionV3
    m, sd = net
    full = tmp_path / "inception.pth"
    torch.save(m.state_dict(), full)
    bare = tmp_path / "inception_bare.pth"
    torch.save({k: v for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}, bare)
    for path in (full, bare):
        m2 = FIDInceptionV3(ckpt=str(path))
        for k, v in m2.state_dict().items():
            if not k.endswith("num_batches_tracked"):
                assert torch.equal(v, sd[k]), k
        assert not m2.training
    broken = tmp_path / "broken.pth"
    torch.save({k: v for k, v in m.state_dict().items() if k != "Mixed_6a.branch3x3.conv.weight"}, broken)
    with pytest.raises(KeyError, match="Mixed_6a.branch3x3.conv.weight"):
        FIDInceptionV3(ckpt=str(broken))
    extra = tmp_path / "extra.pth"
    torch.save(dict(m.state_dict(), **{"AuxLogits.conv0.conv.weight": torch.zeros(1)}), extra)
    with pytest.raises(KeyError, match="AuxLogits.conv0.conv.weight"):
        FIDInceptionV3(ckpt=str(extra))
    assert FIDInceptionV3(resolution=107).resolution == 107 and m.resolution == 299
    with pytest.raises(ValueError, match="without an output pixel"):
        FIDInceptionV3(resolution=40)


def test_refusals(net):
    from frido_amd import fid, pipeline
    m, _ = net
    with pytest.raises(NotImplementedError, match="forward-only"):
        m.train()
    assert m.eval() is m and not m.training
    for bad in (torch.zeros(2, 3, 8, 8, dtype=torch.float64), torch.zeros(2, 8, 8, 3), torch.zeros(2, 3, 8, 8, dtype=torch.uint8),
                torch.zeros(2, 8, 8, 4, dtype=torch.uint8), torch.zeros(2, 4, 8, 8), torch.zeros(3, 8, 8), "x", torch.zeros(0, 3, 8, 8)):
        with pytest.raises(ValueError, match="uint8 .B, H, W, 3. or float32 .B, 3, H, W."):
            m(bad)
    with pytest.raises(ValueError, match="quant"):
        m(torch.zeros(1, 3, 8, 8), quant="round")
    for ok_but_cpu in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(FridoHipError, match="no CPU fallback"):
            m(ok_but_cpu)
    st = fid.FeatureStatistics(8, "cpu")
    with pytest.raises(FridoHipError, match="no CPU fallback"):
        st.update(torch.zeros(2, 8))
    for bad in (torch.zeros(2, 4), torch.zeros(8), torch.zeros(2, 8, dtype=torch.float64), None):
        with pytest.raises(ValueError, match="float32"):
            st.update(bad)
    with pytest.raises(ValueError, match="at least 2 samples"):
        st.cov()
    with pytest.raises(ValueError, match="no features"):
        st.mean()
    with pytest.raises(ValueError, match="FIDInceptionV3"):
        pipeline.fid_statistics(object(), torch.zeros(1, 3, 8, 8))
    with pytest.raises(ValueError, match="FeatureStatistics"):
        pipeline.fid_statistics(m, torch.zeros(1, 3, 8, 8), stats=3)
    with pytest.raises(ValueError, match="one D"):
        fid.frechet_distance(torch.zeros(4), torch.eye(4), torch.zeros(5), torch.eye(5))
    with pytest.raises(ValueError, match="one D"):
        fid.frechet_distance(torch.zeros(4), torch.eye(4), torch.zeros(4), torch.eye(5))
    with pytest.raises(ValueError, match="nothing to merge"):
        fid.FeatureStatistics.merge([])
    with pytest.raises(ValueError, match="widths differ"):
        fid.FeatureStatistics.merge([fid.FeatureStatistics(4, "cpu"), fid.FeatureStatistics(8, "cpu")])


# ---- statistics -------------------------------------------------------------------------------------------
def _stats_of(x, device="cpu"):
    """FeatureStatistics holding the in-order float64 sums of x [N, D] float32 (what update() leaves on the GPU)."""
    from frido_amd import fid
    st = fid.FeatureStatistics(x.shape[1], device)
    st.s1, st.s2 = R.accumulate(x)
    st.n = x.shape[0]
    return st


def _features(tag, N, D, spread=True):
    """N x D float32 features of full rank with correlated columns, distinct variances and a non-zero mean, like pooled post-ReLU
    activations.  The mixing matrix is the identity plus half a random one, so the covariance stays well conditioned (a square random
    matrix alone has singular values down to 1 / D, and a square root's error grows with the inverse of the eigenvalue)."""
    g = synth.seeded_normal(tag, (N, D)).astype(np.float64)
    mix = np.eye(D) + 0.5 * synth.seeded_normal(tag + ":mix", (D, D)).astype(np.float64) / np.sqrt(D)
    scale = np.linspace(0.5, 2.0, D) if spread else 1.0
    return torch.from_numpy(((g @ mix) * scale + 0.5 + np.linspace(0, 1, D)).astype(np.float32))


def test_cov_from_streaming_sums_against_numpy():
    """sigma = (s2 - n mu mu^T) / (n - 1) against np.cov.  Both terms are about n max(x^2) large and each is a float64 sum of n terms
    (error <= n 2^-53 per unit in the worst case, the products being exact), their difference is divided by n - 1: the bound is
    4 n 2^-53 max(x^2).  Measured when written: 100 x to 1000 x inside it."""
    for N, D in ((64, 16), (500, 32), (4096, 8)):
        x = _features(f"fid:cov{N}", N, D)
        st = _stats_of(x)
        mu, cov = R.mean_cov(x.numpy())
        bound = 4 * N * 2.0 ** -53 * float(x.double().pow(2).max())
        e_cov = float(np.abs(st.cov().numpy() - cov).max())
        e_mu = float(np.abs(st.mean().numpy() - mu).max())
        print(f"N = {N}, D = {D}: cov error {e_cov:.2e}, mean error {e_mu:.2e}, bound {bound:.2e}")
        assert e_cov <= bound and e_mu <= bound
        assert torch.equal(st.s2, st.s2.T)


def test_merge_in_order_save_and_load(tmp_path):
    from frido_amd import fid
    x = _features("fid:merge", 96, 16)
    parts = [_stats_of(x[:32]), _stats_of(x[32:40]), _stats_of(x[40:])]
    m = fid.FeatureStatistics.merge(parts)
    assert m.n == 96
    assert torch.equal(m.s1, (parts[0].s1 + parts[1].s1) + parts[2].s1) and torch.equal(m.s2, (parts[0].s2 + parts[1].s2) + parts[2].s2)
    whole = _stats_of(x)
    assert float((m.cov() - whole.cov()).abs().max()) <= 4 * 96 * 2.0 ** -53 * float(x.double().pow(2).max())
    assert parts[0].n == 32 and torch.equal(parts[0].s1, R.accumulate(x[:32])[0])      # the parts are left as they were
    path = tmp_path / "stats.npz"
    whole.save(str(path))
    z = np.load(path)
    assert set(z.files) == {"mu", "sigma", "n"} and int(z["n"]) == 96 and z["mu"].dtype == np.float64 and z["sigma"].shape == (16, 16)
    back = fid.FeatureStatistics.load(str(path))
    assert back.n == 96 and back.D == 16
    tol = 8 * 96 * 2.0 ** -53 * float(x.double().pow(2).max())
    assert float((back.mean() - whole.mean()).abs().max()) <= tol and float((back.cov() - whole.cov()).abs().max()) <= tol
    assert abs(fid.frechet_distance(back.mean(), back.cov(), whole.mean(), whole.cov())) <= 1e-12 * float(torch.trace(whole.cov()))


GATHER_WORKER = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import inception_ref as R
from frido_amd import fid
from test_fid_host import _features, _stats_of
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
x = _features("fid:gather", 40, 8)
cut = [0, 17, 40]
mine = _stats_of(x[cut[rank]:cut[rank + 1]])
full = mine.all_gather_merge()
want = fid.FeatureStatistics.merge([_stats_of(x[cut[r]:cut[r + 1]]) for r in range(world)])      # rank order
assert full.n == 40 and torch.equal(full.s1, want.s1) and torch.equal(full.s2, want.s2), rank
assert mine.n == cut[rank + 1] - cut[rank]
dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_all_gather_merge_world_size_2_gloo(tmp_path):
    from frido_amd import fid
    st = _stats_of(_features("fid:alone", 8, 4))
    assert st.all_gather_merge() is st                                       # no process group: nothing to gather
    script = tmp_path / "worker.py"
    script.write_text(GATHER_WORKER % (REPO, REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29531", str(script)],
                         capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("ok") == 2


# ---- the distance -----------------------------------------------------------------------------------------
# |symmetric route - sqrtm route| / distance, measured when this test was written (float64, this file's features):
#   D = 16, N = 128: 8.82e-16      D = 32, N = 256: 1.01e-15      (one to four units in the last place of a distance of 16 / 28)
SQRTM_MEASURED = {16: 8.82e-16, 32: 1.01e-15}


@pytest.mark.parametrize("D", [16, 32])
def test_frechet_distance_against_scipy_sqrtm(D):
    """The symmetric route against torch-fidelity's formula, scipy.linalg.sqrtm(sigma1 @ sigma2), at full rank (N = 8 D).  The bound is
    10 x the disagreement measured when written (SQRTM_MEASURED; ten for platform BLAS differences).  No rank-deficient case is held to
    sqrtm: there it is sqrtm that is off (1.6e-9)."""
    from frido_amd import fid
    a, b = _features(f"fid:fa{D}", 8 * D, D), _features(f"fid:fb{D}", 8 * D, D, spread=False) * 1.25 + 0.1
    (m1, c1), (m2, c2) = R.mean_cov(a.numpy()), R.mean_cov(b.numpy())
    ours = fid.frechet_distance(torch.from_numpy(m1), torch.from_numpy(c1), torch.from_numpy(m2), torch.from_numpy(c2))
    ref = R.frechet_sqrtm(m1, c1, m2, c2)
    rel = abs(ours - ref) / abs(ref)
    print(f"D = {D}: symmetric {ours:.17g}, sqrtm {ref:.17g}, relative difference {rel:.2e}")
    assert ref > 0.1 and rel <= 10 * SQRTM_MEASURED[D]
    # numpy inputs and a swap of the two sides give the same distance
    assert fid.frechet_distance(m1, c1, m2, c2) == ours
    assert abs(fid.frechet_distance(m2, c2, m1, c1) - ours) <= 1e-12 * abs(ours)


@pytest.mark.parametrize("D", [16, 32, 64])
def test_frechet_distance_of_a_distribution_to_itself(D):
    """|d(s, s)| <= 1e-12 tr(sigma) at full rank, and the result is not clamped (1.3e-15 .. 2.0e-15 of the trace when written)."""
    from frido_amd import fid
    x = _features(f"fid:self{D}", 8 * D, D)
    m, c = R.mean_cov(x.numpy())
    d = fid.frechet_distance(torch.from_numpy(m), torch.from_numpy(c), torch.from_numpy(m), torch.from_numpy(c))
    print(f"D = {D}: d(s, s) = {d:.3e}, tr = {np.trace(c):.3e}, ratio {abs(d) / np.trace(c):.2e}")
    assert abs(d) <= 1e-12 * np.trace(c)
    # a rank-deficient covariance (N < D) is handled by the clamp, without an eps offset.  Its null eigenvalues come out of eigvalsh as
    # rounding noise of the order 2^-53 lambda_max^2 (of r sigma r), and the square root of that is 2^-26.5 lambda_max per null
    # direction: at most D 2^-26 tr(sigma) in all -- the square root's own conditioning at zero, whatever the route
    y = _features(f"fid:low{D}", D // 2, D)
    m, c = R.mean_cov(y.numpy())
    d = fid.frechet_distance(m, c, m, c)
    print(f"D = {D}, rank {D // 2 - 1}: d(s, s) = {d:.3e}, ratio {abs(d) / np.trace(c):.2e}")
    assert abs(d) <= D * 2.0 ** -26 * np.trace(c)
    # a pure shift of the mean: the distance is |shift|^2 on top of that
    d2 = fid.frechet_distance(m, c, m + 0.5, c)
    assert abs(d2 - d - 0.25 * D) <= 1e-12 * max(np.trace(c), 0.25 * D)


def test_frechet_distance_is_not_clamped():
    """A pair whose value by the function's definition is negative, exactly: sigma = diag(1, -e), a covariance with an eigenvalue that
    rounding pushed below zero.  The clamp makes r = diag(1, 0) and r sigma r = diag(1, 0), so the last term is 2 and the distance is
    2 (1 - e) - 2 = -2 e.  A clamped result would be 0."""
    from frido_amd import fid
    e = 2.0 ** -20
    sigma = torch.diag(torch.tensor([1.0, -e], dtype=torch.float64))
    mu = torch.zeros(2, dtype=torch.float64)
    d = fid.frechet_distance(mu, sigma, mu, sigma)
    assert d < 0 and abs(d + 2 * e) <= 8 * 2.0 ** -52


# ---- ABI --------------------------------------------------------------------------------------------------
def test_descriptors_match_both_builds_and_bad_ones_are_turned_away():
    from frido_amd import fid
    buf = (C.c_double * 64)()
    base = (C.addressof(buf) + 15) & ~15
    for planes in ("f16", "bf16"):
        L = _lib.lib(planes)
        for name, (struct, sizeof) in fid.LAUNCHERS.items():
            assert getattr(L, sizeof)() == C.sizeof(struct), (planes, name)
        fns = fid._fns(planes)
        assert set(fns) == set(fid.LAUNCHERS)

        def refused(name, desc, words):
            assert fns[name](C.byref(desc), None) == -1 and words in L.frido_last_error(), (name, L.frido_last_error())      # FRIDO_EINVAL

        for name, (struct, _) in fid.LAUNCHERS.items():                      # a zeroed descriptor: null pointers
            refused(name, struct(), name.encode() + b": bad arguments")
        for kw, words in ((dict(S=0), b"bad arguments"), (dict(src_kind=2), b"src_kind"), (dict(quant=0), b"quant"), (dict(dst=base + 4), b"16-byte")):
            d = fid.preprocess_desc(base, base, 1, 4, 4, 4, src_kind=fid.SRC_F32_NCHW)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_fid_preprocess", d, words)
        for kw, words in ((dict(C=6), b"multiples of 4"), (dict(mode=3), b"mode"), (dict(H=2, mode=0), b"3 x 3 window"), (dict(c0=8, ldd=8), b"inside ldd"),
                          (dict(ldd=10), b"multiples of 4"), (dict(c0=2), b"multiples of 4"), (dict(src=base + 8), b"16-byte"), (dict(B=0), b"bad arguments")):
            d = fid.pool_desc(base, base, 1, 4, 4, 8, fid.POOL_AVG_S1P1)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_pool3", d, words)
        for kw, words in ((dict(C=6), b"multiple of 4"), (dict(HW=0), b"bad arguments"), (dict(dst=base + 4), b"16-byte")):
            d = fid.gap_desc(base, base, 1, 4, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_gap", d, words)
        for kw, words in ((dict(D=6), b"multiple of 4"), (dict(B=0), b"bad arguments"), (dict(s2=base + 4), b"aligned"), (dict(s1=None), b"bad arguments")):
            d = fid.accum_desc(base, base, base, 1, 8)
            for k, v in kw.items():
                setattr(d, k, v)
            refused("frido_feat_accum", d, words)
    assert fid.QUANT == {"pil": 2, "np": 1}                                  # FridoGemm.u8_mode's numbers


def test_the_op_table_header_does_not_know_the_launches():
    """frido_hip.h is the op-kind ABI (tests/test_opkinds_host.py pins it): the FID launches live in a header of their own, in a source
    file that includes launch.h alone and sits directly behind patchgan.hip."""
    hip = open(os.path.join(REPO, "include", "frido_hip.h")).read()
    for name in ("fid", "pool3", "FridoGap", "FridoFeatAccum", "frido_gap", "feat_accum"):
        assert name not in hip
    assert _lib.ABI_VERSION == 8 and _lib.OP_KINDS["FRIDO_OP__COUNT"] == 36
    assert not [s for s in _lib.EXPORTS if "fid" in s or "pool3" in s or "gap" in s or "feat_accum" in s]
    assert not [s for s in _lib.STRUCTS if "Fid" in s or "Pool3" in s or "Gap" in s or "FeatAccum" in s]
    hdr = open(os.path.join(REPO, "include", "frido_fid.h")).read()
    body = _lib._strip_comments(hdr)
    assert body.split("#include")[1].strip().startswith('"frido_hip.h"')      # the first include
    assert _lib._parse_structs(body).keys() == {"FridoFidPreprocess", "FridoPool3", "FridoGap", "FridoFeatAccum"}
    mk = open(os.path.join(REPO, "frido_amd", "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS")][0].split()
    assert srcs[-1] == "lpips.hip" and srcs[-2] == "vision.hip"              # the status words are numbered in link order
    assert srcs[srcs.index("patchgan.hip") + 1] == "fid.hip"
    assert "fid.o obj_bf16p/fid.o: ../../include/frido_fid.h" in mk
    src = open(os.path.join(REPO, "frido_amd", "csrc", "fid.hip")).read()
    assert '#include "launch.h"' in src and "common.h" not in src
    low = src.lower()
    for word in ("atomic", "hipmalloc", "hipfree", "synchronize", "status_raise", "__syncthreads"):
        assert word not in low, word


def test_builder_conv_padx_leaves_existing_geometries_alone():
    """Builder.conv(padx=None) emits the geometry it always did (no padx key: Prog.gemm fills in pad); padx= sets the left padding and
    the output width follows it."""
    import inspect
    from frido_amd.builder import Builder
    sig = inspect.signature(Builder.conv)
    assert sig.parameters["padx"].default is None and sig.parameters["padx"].kind is inspect.Parameter.KEYWORD_ONLY
    seen = []

    class FakeProg:
        ops = []

        def gemm(self, M, N, K, a, wop, **kw):
            seen.append((M, N, K, kw["conv"]))

    b = Builder.__new__(Builder)
    b.w = {"c.weight": torch.zeros(8, 32, 1, 7)}
    b.conv_weight = lambda name: (None, 32)
    b.bias = lambda name: None
    b.prog = FakeProg()
    b.f32_strict = lambda M, N: type("T", (), dict(ptr=0, C=N))()
    a = type("A", (), dict(K=32))()
    b.conv(a, 1, 5, 5, "c", pad=0, padx=3, out="f32_strict")
    b.conv(a, 1, 5, 9, "c", pad=0, out="f32_strict")
    (M1, _, K1, g1), (M2, _, _, g2) = seen
    assert g1["pad"] == 0 and g1["padx"] == 3 and (g1["Ho"], g1["Wo"]) == (5, 5) and M1 == 25 and K1 == 7 * 32
    assert "padx" not in g2 and (g2["Ho"], g2["Wo"]) == (5, 3) and M2 == 15


def test_fid_npy_tool_on_saved_statistics(tmp_path):
    """tools/fid_npy.py on two .npz statistics files needs no GPU and prints the distance frechet_distance returns."""
    from frido_amd import fid
    a, b = _stats_of(_features("fid:tool:a", 64, 8)), _stats_of(_features("fid:tool:b", 64, 8, spread=False) * 1.5)
    pa, pb = tmp_path / "a.npz", tmp_path / "b.npz"
    a.save(str(pa))
    b.save(str(pb))
    out = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fid_npy.py"), str(pa), str(pb)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = fid.frechet_distance(a.mean(), a.cov(), b.mean(), b.cov())
    assert out.stdout.startswith("frechet_distance ") and "n = 64 / 64" in out.stdout
    assert abs(float(out.stdout.split()[1]) - want) <= 1e-6 * want + 1e-6
    bad = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fid_npy.py"), str(pa), str(tmp_path / "none.npy")], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "no such file" in bad.stderr
