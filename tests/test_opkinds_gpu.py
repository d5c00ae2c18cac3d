"""The nine op kinds of ABI 8 on the device: for each, descriptors at the smallest shapes that reach each of its code paths, run three ways
-- through the exported launcher, as an op of a Prog via run, and captured with Prog.capture and launched twice on fresh inputs at the
captured addresses -- with bit-equal outputs (torch.equal); and a mixed program through run_timed."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from frido_amd import _lib, patching  # noqa: E402
from frido_amd.engine import Prog, require_gpu  # noqa: E402
from frido_amd.synth import seeded_normal  # noqa: E402


class Case:
    """One descriptor over buffers of its own.  ins: float tensors refilled per round (the fresh inputs); state: float tensors refilled per
    round that the kernel updates in place; outs: tensors the kernel writes (reset to a sentinel per round).  state + outs are compared."""

    def __init__(self, kind, fields, ins=(), state=(), outs=(), keep=()):
        self.kind, self.ins, self.state, self.outs, self.keep = kind, list(ins), list(state), list(outs), list(keep)
        self.op = fields if isinstance(fields, tuple) else _lib.make_op(kind, **fields)      # a finished op (_lib.op_of), or the fields

    def reset(self, tag, rnd):
        for i, t in enumerate(self.ins + self.state):
            t.copy_(torch.from_numpy(seeded_normal(f"opkinds:{tag}:{i}:{rnd}", tuple(t.shape))))
        for t in self.outs:
            t.fill_(0 if t.dtype == torch.uint8 else -7.0)

    def results(self):
        return [t.clone() for t in self.state + self.outs]


def _f(*shape):
    return torch.zeros(*shape, dtype=torch.float32, device="cuda")


def _p(t):
    return t.data_ptr() if t is not None else None


# ---- the descriptors ----------------------------------------------------------------------------------------------------------------
def dpm_step(Bk, HW, Cx, start, nch, row):
    x, ec, eu, hist, p0 = _f(Bk, HW, Cx), _f(Bk * HW, nch), _f(Bk * HW, nch), _f(Bk * HW, nch), _f(Bk, HW, Cx)
    #                      inv_alpha sigma c_x  c_d   w_cur w_last: row 0 first order (x0_hist not read), row 1 second order
    coef = torch.tensor([[1.25, 0.6, 0.8, 0.3, 1.0, 0.0, 0, 0], [1.1, 0.4, 0.9, 0.2, 1.5, -0.5, 0, 0]], device="cuda")
    return Case("FRIDO_OP_DPM_STEP", dict(x=_p(x), B=Bk, HW=HW, Cx=Cx, start=start, nch=nch, eps_cond=_p(ec), eps_uncond=_p(eu), cfg_scale=2.0,
                                          coef=_p(coef), coef_row_offset=row, x_out=_p(x), pred_x0=_p(p0), x0_hist=_p(hist)),
                ins=[ec, eu], state=[x, hist], outs=[p0], keep=[coef])


def keep_blend(noise, masked, clean=False):
    Bk, HW, Cx, c0, c1 = 2, 16, 6, 3, 6
    x, z0 = _f(Bk, HW, Cx), _f(Bk, HW, Cx)
    mask = torch.from_numpy(seeded_normal("opkinds:mask", (Bk, HW))).cuda().sigmoid() if masked else None
    qtab = torch.tensor([[0.9, 0.2], [0.6, 0.7]], device="cuda")
    kw = dict(x=_p(x), z0=_p(z0), mask=_p(mask), B=Bk, HW=HW, Cx=Cx, c0=c0, c1=c1, clean=int(clean))
    ins = [z0]
    if not clean:
        kw.update(qtab=_p(qtab), row_offset=1)
        if noise == "tape":
            tape = _f(1, Bk, HW, Cx)
            kw.update(noise=_p(tape), noise_stride=Bk * HW * Cx, noise_C=Cx)
            ins.append(tape)
        else:
            kw.update(seed=5, sample0=3, rng_stream=65)
    return Case("FRIDO_OP_KEEP_BLEND", kw, ins=ins, state=[x], keep=[mask, qtab])


def invert_step(cfg):
    Bk, HW, Cx, lo, hi = 2, 16, 6, 3, 6
    x, ec, eu = _f(Bk, HW, Cx), _f(Bk * HW, hi - lo), _f(Bk * HW, hi - lo)
    coef = torch.tensor([[1.02, 0.05], [1.05, 0.11]], device="cuda")
    return Case("FRIDO_OP_INVERT_STEP", dict(x=_p(x), eps_cond=_p(ec), eps_uncond=_p(eu) if cfg else None, cfg_scale=2.0, coef=_p(coef),
                                             coef_row_offset=1, B=Bk, HW=HW, Cx=Cx, c_lo=lo, c_hi=hi),
                ins=[ec, eu], state=[x], keep=[coef])


def guidance_compose(per_sample, rescale):
    n, Bk = 3, 2
    eps = _f(n + 1, Bk * per_sample)      # composed in place into slot 0, as the engine does
    w = torch.tensor([1.5, -0.75, 0.5, 0.5], device="cuda")      # w_0 .. w_2, phi
    return Case("FRIDO_OP_GUIDANCE_COMPOSE", dict(eps=_p(eps), out=_p(eps), weights=_p(w), n=n, B=Bk, per_sample=per_sample, rescale=rescale),
                state=[eps], keep=[w])


def _geo():
    return patching.geometry(dict(vqf=4, patch_distributed_vq=True, clip_min_weight=0.01, clip_max_weight=0.5, clip_min_tie_weight=0.01,
                                  clip_max_tie_weight=0.5, ks=(8, 8), stride=(4, 4), tie_braker=True), 16, 16, patching.MODEL, torch.device("cuda"))


def unfold():
    geo, Bk, Cn = _geo(), 2, 6
    src, crops = _f(Bk, 16, 16, Cn), _f(Bk * geo.L, 8, 8, Cn)
    return Case("FRIDO_OP_UNFOLD", _lib.op_of("FRIDO_OP_UNFOLD", geo.unfold_desc(_p(src), _p(crops), Bk, Cn)), ins=[src], outs=[crops], keep=[geo])


def fold(u8):
    geo, Bk, Cn = _geo(), 2, 6
    crops = _f(Bk * geo.L, 8, 8, Cn)
    out = torch.zeros(Bk, 16, 16, Cn, dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    desc = geo.fold_desc(_p(crops), None, Bk, Cn, out_u8=_p(out), u8_mode=1) if u8 else geo.fold_desc(_p(crops), _p(out), Bk, Cn)
    return Case("FRIDO_OP_FOLD", _lib.op_of("FRIDO_OP_FOLD", desc), ins=[crops], outs=[out], keep=[geo])


OBJ = dict(B=2, HW=16, Cx=8, T=10)
T_IDX = [3, 8]


def _schedule():
    ac = torch.linspace(0.95, 0.05, OBJ["T"], device="cuda")
    return ac.sqrt().contiguous(), (1 - ac).sqrt().contiguous()


def qsample(tape):
    Bk, HW, Cx = OBJ["B"], OBJ["HW"], OBJ["Cx"]
    x0, xn, noise = _f(Bk, HW, Cx), _f(Bk, HW, 8), _f(Bk, HW, Cx)
    t, (sa, sb) = torch.tensor(T_IDX, dtype=torch.int64, device="cuda"), _schedule()
    kw = dict(x0=_p(x0), x_noisy=_p(xn), t=_p(t), sqrt_ac=_p(sa), sqrt_1mac=_p(sb), mix_tau=0.1, ch_start=4, ch_end=8, rng_stream=1, **OBJ)
    kw.update(dict(noise=_p(noise)) if tape else dict(seed=9, sample0=2))
    return Case("FRIDO_OP_QSAMPLE", kw, ins=[x0] + ([noise] if tape else []), outs=[xn], keep=[t, sa, sb])


def diffusion_loss(tape):
    Bk, HW, Cx = OBJ["B"], OBJ["HW"], OBJ["Cx"]
    pred, noise, per, row = _f(Bk, HW, 4), _f(Bk, HW, Cx), _f(Bk), _f(4)
    t = torch.tensor(T_IDX, dtype=torch.int64, device="cuda")
    logvar, lvlb = torch.linspace(-0.5, 0.5, OBJ["T"], device="cuda"), torch.linspace(0.1, 2.0, OBJ["T"], device="cuda")
    kw = dict(pred=_p(pred), t=_p(t), logvar=_p(logvar), lvlb_weights=_p(lvlb), per_sample=_p(per), out=_p(row), ch_start=4, nch=4, rng_stream=1,
              loss_type=1, l_simple_weight=1.0, original_elbo_weight=0.5, **OBJ)
    kw.update(dict(noise=_p(noise)) if tape else dict(seed=9, sample0=2))
    return Case("FRIDO_OP_DIFFUSION_LOSS", kw, ins=[pred] + ([noise] if tape else []), outs=[per, row], keep=[t, logvar, lvlb])


def vq_commit_loss(scales):
    """scales: (pixels, C, c0, e) per scale, coarse first."""
    from frido_amd.vqloss import commit_loss_desc
    z, zq = [_f(n, Cn) for n, Cn, _, _ in scales], [_f(n, Cn) for n, Cn, _, _ in scales]
    partials = torch.zeros(_lib.VQLOSS_WS_BYTES // 8, dtype=torch.float64, device="cuda")
    means, total = _f(len(scales)), _f(1)
    desc = commit_loss_desc([(_p(a), _p(b), n, Cn, c0, e) for a, b, (n, Cn, c0, e) in zip(z, zq, scales)], partials=_p(partials), out=_p(means),
                            emb_loss=_p(total), beta=0.25, legacy=True)
    return Case("FRIDO_OP_VQ_COMMIT_LOSS", _lib.op_of("FRIDO_OP_VQ_COMMIT_LOSS", desc), ins=z + zq, outs=[means, total], keep=[partials])


CASES = {
    "dpm_vec_first": lambda: dpm_step(2, 16, 8, 4, 4, 0), "dpm_vec_second": lambda: dpm_step(2, 16, 8, 4, 4, 1),
    "dpm_scalar_first": lambda: dpm_step(2, 16, 6, 3, 3, 0), "dpm_scalar_second": lambda: dpm_step(2, 16, 6, 3, 3, 1),
    "blend_philox_masked": lambda: keep_blend("philox", True), "blend_philox_unmasked": lambda: keep_blend("philox", False),
    "blend_tape_masked": lambda: keep_blend("tape", True), "blend_tape_unmasked": lambda: keep_blend("tape", False),
    "blend_clean": lambda: keep_blend(None, True, clean=True),
    "invert_cfg": lambda: invert_step(True), "invert_plain": lambda: invert_step(False),
    "compose_vec": lambda: guidance_compose(104, 0), "compose_scalar": lambda: guidance_compose(105, 0),
    "compose_vec_rescale": lambda: guidance_compose(104, 1), "compose_scalar_rescale": lambda: guidance_compose(105, 1),
    "unfold": unfold, "fold_f32": lambda: fold(False), "fold_u8": lambda: fold(True),
    "qsample_tape": lambda: qsample(True), "qsample_philox": lambda: qsample(False),
    "loss_tape": lambda: diffusion_loss(True), "loss_philox": lambda: diffusion_loss(False),
    "vqloss_two_scales_e3": lambda: vq_commit_loss([(4, 3, 0, 3), (16, 3, 0, 3)]), "vqloss_one_scale_e4": lambda: vq_commit_loss([(16, 8, 4, 4)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_launcher_run_and_captured_graph_agree_bit_for_bit(name):
    dev = require_gpu("cuda")
    case = CASES[name]()
    kind, st = case.op
    launcher = getattr(_lib.lib(), "frido_" + case.kind[len("FRIDO_OP_"):].lower())
    prog = Prog(dev, 2)
    prog.ops.append(case.op)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = side.cuda_stream
        want = []
        for rnd in (0, 1):                   # 1. the exported launcher, on two sets of inputs
            case.reset(name, rnd)
            _lib.check(launcher(C.byref(st), sp), case.kind)
            want.append(case.results())
        assert not all(torch.equal(a, b) for a, b in zip(*want)), "the two rounds must differ"
        assert all(bool(torch.isfinite(t.float()).all()) for r in want for t in r)
        case.reset(name, 0)                  # 2. an op of a program
        prog.run(sp)
        got = case.results()
        assert all(torch.equal(a, b) for a, b in zip(got, want[0])), "Prog.run"
        graph = prog.capture(sp)             # 3. captured, launched twice on fresh inputs at the captured addresses
        for rnd in (0, 1):
            case.reset(name, rnd)
            graph.launch(sp)
            got = case.results()
            assert all(torch.equal(a, b) for a, b in zip(got, want[rnd])), f"graph launch {rnd}"
        side.synchronize()
    torch.cuda.current_stream().wait_stream(side)


def test_run_timed_times_every_op_of_a_mixed_program():
    """[UNFOLD, COPY, FOLD, STEP_ADD]: run_timed returns one finite, non-negative time per op and leaves what run leaves."""
    dev = require_gpu("cuda")
    geo, Bk, Cn = _geo(), 2, 6
    xs = torch.from_numpy(seeded_normal("opkinds:timed", (Bk, 16, 16, Cn))).cuda()
    crops = _f(Bk * geo.L, 8, 8, Cn)
    moved, out = torch.zeros_like(crops), _f(Bk, 16, 16, Cn)
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    prog = Prog(dev, 2)
    prog.ops.append(_lib.op_of("FRIDO_OP_UNFOLD", geo.unfold_desc(_p(xs), _p(crops), Bk, Cn)))
    prog.emit("FRIDO_OP_COPY", src=_p(crops), dst=_p(moved), n=crops.numel() * 4)
    prog.ops.append(_lib.op_of("FRIDO_OP_FOLD", geo.fold_desc(_p(moved), _p(out), Bk, Cn)))
    prog.emit("FRIDO_OP_STEP_ADD", step=_p(step), delta=1)
    sp = torch.cuda.current_stream().cuda_stream
    prog.run(sp)
    torch.cuda.synchronize()
    want = out.clone()
    out.zero_()
    ms = prog.run_timed(sp)
    torch.cuda.synchronize()
    assert len(ms) == len(prog.ops) == 4 and all(math.isfinite(v) and v >= 0 for v in ms), ms
    assert torch.equal(out, want) and int(step) == 2 and bool(want.abs().max() > 0)
