"""Host-side noise schedules (numpy).  Scalars only — nothing here touches image data.

Restates, with the reference's exact float32/float64 mix so tables are bit-identical
(pinned by tests/golden/schedules.npz):
  frido/modules/diffusionmodules/util.py:21-26   make_beta_schedule('linear')
  frido/models/diffusion/frido.py:127-168        register_schedule (float64 cumprod -> float32 buffers, posterior q(x_{t-1} | x_t, x_0))
  frido/modules/diffusionmodules/util.py:46-74   make_ddim_timesteps / make_ddim_sampling_parameters
  frido/models/diffusion/ddim.py:25-54           DDIMSampler.make_schedule
"""
import numpy as np

COEF_ROW = 12   # must match csrc/misc.hip: a_t, a_prev, sigma, sqrt(1-a_t), ab0..ab3, den, pad
                # (FRIDO_STEP_ANCESTRAL rows: sqrt_recip_ac, sqrt_recipm1_ac, post_coef1, post_coef2, sigma, clip, pad)


def _linspace(start, end, steps):
    """torch.linspace's float64 evaluation (what the reference's schedule is built with): symmetric — first half
    fma(step, i, start), second half fma(-step, steps-1-i, end) — with FUSED multiply-adds, emulated here through
    80-bit long doubles (the product step*i is exact in 64 mantissa bits for i < 2^11).  np.linspace differs in
    the last bit for ~15 % of the entries."""
    L = np.longdouble
    start, end = np.float64(start), np.float64(end)
    step = (end - start) / np.float64(steps - 1)
    i = np.arange(steps)
    lo = (L(step) * i.astype(L) + L(start)).astype(np.float64)
    hi = (L(end) - L(step) * (steps - 1 - i).astype(L)).astype(np.float64)
    return np.where(i < steps // 2, lo, hi)


def make_beta_schedule(schedule, n_timestep, linear_start=1e-4, linear_end=2e-2, cosine_s=8e-3):
    if schedule == "linear":
        return _linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep) ** 2
    if schedule == "sqrt_linear":
        return _linspace(linear_start, linear_end, n_timestep)
    if schedule == "sqrt":
        return _linspace(linear_start, linear_end, n_timestep) ** 0.5
    if schedule == "cosine":
        ts = np.arange(n_timestep + 1, dtype=np.float64) / n_timestep + cosine_s
        al = np.cos(ts / (1 + cosine_s) * np.pi / 2) ** 2
        al = al / al[0]
        return np.clip(1 - al[1:] / al[:-1], 0, 0.999)
    raise ValueError(f"schedule '{schedule}' unknown.")


def ddpm_tables(betas, v_posterior=0.):
    """The float32 buffers DDPM.register_schedule registers (inference subset), the posterior q(x_{t-1} | x_t, x_0) of frido.py:157-168
    included: float64 arithmetic in the reference's order of operations, one cast to float32 at the end."""
    betas = np.asarray(betas, dtype=np.float64)
    alphas = 1.0 - betas
    ac = np.cumprod(alphas, axis=0)
    ac_prev = np.append(1.0, ac[:-1])
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    post_var = (1 - v_posterior) * betas * (1. - ac_prev) / (1. - ac) + v_posterior * betas
    return dict(betas=f32(betas), alphas_cumprod=f32(ac), alphas_cumprod_prev=f32(ac_prev),
                sqrt_alphas_cumprod=f32(np.sqrt(ac)), sqrt_one_minus_alphas_cumprod=f32(np.sqrt(1.0 - ac)),
                log_one_minus_alphas_cumprod=f32(np.log(1.0 - ac)), sqrt_recip_alphas_cumprod=f32(np.sqrt(1.0 / ac)),
                sqrt_recipm1_alphas_cumprod=f32(np.sqrt(1.0 / ac - 1)),
                posterior_variance=f32(post_var),
                # (clipped: the posterior variance is 0 at t = 0)
                posterior_log_variance_clipped=f32(np.log(np.maximum(post_var, 1e-20))),
                posterior_mean_coef1=f32(betas * np.sqrt(ac_prev) / (1. - ac)),
                posterior_mean_coef2=f32((1. - ac_prev) * np.sqrt(alphas) / (1. - ac)))


def ancestral_table(tables, T=None, clip_denoised=False):
    """float32 table [T][COEF_ROW] of the ancestral (DDPM) update in LOOP order -- row i is the step at t = T - 1 - i, the order of
    `reversed(range(T))` in frido.py:1391-1394 -- for FridoSamplerStep.hist_mode = FRIDO_STEP_ANCESTRAL:
    {sqrt_recip_alphas_cumprod[t], sqrt_recipm1_alphas_cumprod[t], posterior_mean_coef1[t], posterior_mean_coef2[t],
     sigma = (t != 0) * exp(0.5 * posterior_log_variance_clipped[t]) (fp32, frido.py:1291,1305), clip (0 / 1), pad}.
    tables: ddpm_tables' dict (or any mapping of the same float32 arrays); T <= len(betas): the chain starts at t = T - 1 (`timesteps=` /
    `start_T` of p_sample_loop)."""
    get = lambda k: np.asarray(tables[k], dtype=np.float32)
    n = get("posterior_mean_coef1").shape[0]
    T = n if T is None else int(T)
    assert 0 < T <= n, f"ancestral_table: T = {T} outside 1 .. {n}"
    t = np.arange(T - 1, -1, -1)
    tab = np.zeros((T, COEF_ROW), dtype=np.float32)
    tab[:, 0] = get("sqrt_recip_alphas_cumprod")[t]
    tab[:, 1] = get("sqrt_recipm1_alphas_cumprod")[t]
    tab[:, 2] = get("posterior_mean_coef1")[t]
    tab[:, 3] = get("posterior_mean_coef2")[t]
    half = (np.float32(0.5) * get("posterior_log_variance_clipped")[t]).astype(np.float32)
    tab[:, 4] = np.exp(half.astype(np.float64)).astype(np.float32) * (t != 0)
    tab[:, 5] = 1.0 if clip_denoised else 0.0
    return tab


def make_ddim_timesteps(method, num_ddim, num_ddpm):
    if method == "uniform":
        ts = np.asarray(list(range(0, num_ddpm, num_ddpm // num_ddim)))
    elif method == "quad":
        ts = (np.linspace(0, np.sqrt(num_ddpm * .8), num_ddim) ** 2).astype(int)
    else:
        raise NotImplementedError(f'There is no ddim discretization method called "{method}"')
    return ts + 1


def make_ddim_sampling_parameters(alphacums32, ddim_timesteps, eta):
    """alphacums32: float32 alphas_cumprod.  Returns (sigmas f64, alphas f32, alphas_prev f64) with the reference's
    exact float mix (util.py:63-74 evaluated on a float32 torch tensor and a float64 ndarray, as ddim.py:43-46 does):
    `ndarray / tensor` dispatches to Tensor.__rtruediv__ = reciprocal(tensor) * ndarray, so 1/(1 - alphas) is formed
    in FLOAT32 and only then widened; everything else is float64."""
    ac = np.asarray(alphacums32, dtype=np.float32)
    alphas = ac[ddim_timesteps]
    alphas_prev = np.asarray([ac[0]] + ac[ddim_timesteps[:-1]].tolist(), dtype=np.float64)
    recip = (np.float32(1.0) / (np.float32(1.0) - alphas)).astype(np.float32).astype(np.float64)
    sigmas = eta * np.sqrt(recip * (1 - alphas_prev) * (1 - alphas.astype(np.float64) / alphas_prev))
    return sigmas, alphas, alphas_prev


def ddim_inversion_table(alphas, alphas_prev):
    """float32 table [n][2] = {c0, c1} of DDIM's deterministic encoder (the probability-flow ODE walked UPWARDS; upstream latent-diffusion's
    DDIMSampler.encode, not in the reference), from the sampler's own ddim_alphas / ddim_alphas_prev (make_schedule(S, ddim_eta=0)).  Row i
    moves the state from level p = alphas_prev[i] to a = alphas[i] with the eps evaluated at ddim_timesteps[i]:
      x' = c0 x + c1 eps,   c0 = sqrt(a / p),   c1 = sqrt(a) (sqrt(1 / a - 1) - sqrt(1 / p - 1))
    -- the exact inverse of the eta = 0 update of the same row with the same eps.  Rows ascend (i = 0 is the first one run); after k rows
    the state sits at alphas[k - 1], where an edit of the chain's last k rows starts.  float64 throughout, rounded to float32 once."""
    a, p = np.asarray(alphas, dtype=np.float64), np.asarray(alphas_prev, dtype=np.float64)
    assert a.shape == p.shape and a.ndim == 1, (a.shape, p.shape)
    return np.stack((np.sqrt(a / p), np.sqrt(a) * (np.sqrt(1.0 / a - 1.0) - np.sqrt(1.0 / p - 1.0))), axis=1).astype(np.float32)


DPM_ROW = 8     # must match csrc/dpmstep.hip: inv_alpha, sigma, c_x, c_d, w_cur, w_last, pad x2
DPM_SKIP_TYPES = ("logSNR", "time_uniform")


def dpm_solver_grid(alphas_cumprod, S, skip_type="logSNR"):
    """(t_loop, ac_cur, ac_next) of the DPM-Solver++ multistep loop, float64: step i evaluates the denoiser at t_loop[i] (descending) and moves
    the state from alphas_cumprod ac_cur[i] to ac_next[i].
    "logSNR": lambda(t) = 0.5 ln(ac_t / (1 - ac_t)); S + 1 targets uniform in lambda from lambda(T - 1) to lambda(0), each snapped to the
    integer t with the nearest lambda (the lowest t on a tie), duplicates removed: T - 1 = t_0 > ... > t_n = 0, n <= S steps ending at ac[0].
    "time_uniform": DDIM's grid -- make_ddim_timesteps("uniform") and the (alphas, alphas_prev) pairs of make_ddim_sampling_parameters."""
    ac = np.asarray(alphas_cumprod, dtype=np.float64)
    T, S = ac.shape[0], int(S)
    if S < 1:
        raise ValueError(f"dpm_solver_table: S = {S}, at least one step is needed")
    if skip_type == "logSNR":
        lam = 0.5 * np.log(ac / (1.0 - ac))
        v = lam[T - 1] + np.arange(S + 1, dtype=np.float64) * ((lam[0] - lam[T - 1]) / S)
        t = np.abs(lam[None, :] - v[:, None]).argmin(axis=1)      # argmin: the first (lowest) t among equals
        t[0], t[-1] = T - 1, 0
        grid = np.asarray(sorted(set(int(k) for k in t), reverse=True), dtype=np.int64)
        t_loop, t_next = grid[:-1], grid[1:]
        ac_cur, ac_next = ac[t_loop], ac[t_next]
    elif skip_type == "time_uniform":
        ts = make_ddim_timesteps("uniform", S, T)
        _, al, alp = make_ddim_sampling_parameters(np.asarray(alphas_cumprod, dtype=np.float32), ts, 0.0)
        t_loop = np.flip(ts).astype(np.int64)
        ac_cur, ac_next = np.flip(al).astype(np.float64), np.flip(alp).astype(np.float64)
    else:
        raise ValueError(f"unknown skip_type {skip_type!r}: one of {DPM_SKIP_TYPES}")
    if t_loop.shape[0] < 1:
        raise ValueError(f"dpm_solver_table: the {skip_type} grid of S = {S} on a schedule of {T} timesteps collapses to no step")
    return t_loop.copy(), ac_cur.copy(), ac_next.copy()


def dpm_solver_rows(ac_cur, ac_next, order=2, lower_order_final=True):
    """The float64 rows [n][DPM_ROW] of DPM-Solver++(2M) (Lu et al. 2022, data prediction, multistep) before rounding.  With
    alpha = sqrt(ac_cur), sigma = sqrt(1 - ac_cur), alpha' / sigma' the same of ac_next, h = ln(alpha' / sigma') - ln(alpha / sigma) and
    r = h_prev / h:   x' = (sigma' / sigma) x - alpha' expm1(-h) D,   D = x0 (first order) or (1 + 1 / 2r) x0 - (1 / 2r) x0_prev.
    Row: {1 / alpha, sigma, c_x = sigma' / sigma, c_d = -alpha' expm1(-h), w_cur, w_last, 0, 0}.  First-order rows (w = 1, 0): row 0 -- every
    stage walks the table from its top with an empty history --, every row when order = 1, the last row under lower_order_final."""
    if order not in (1, 2):
        raise ValueError(f"order = {order!r}: the multistep solver is built for order 1 and 2")
    ac_cur, ac_next = np.asarray(ac_cur, dtype=np.float64), np.asarray(ac_next, dtype=np.float64)
    n = ac_cur.shape[0]
    a, s, a2, s2 = np.sqrt(ac_cur), np.sqrt(1.0 - ac_cur), np.sqrt(ac_next), np.sqrt(1.0 - ac_next)
    h = np.log(a2 / s2) - np.log(a / s)
    rows = np.zeros((n, DPM_ROW), dtype=np.float64)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = 1.0 / a, s, s2 / s, -a2 * np.expm1(-h)
    rows[:, 4] = 1.0
    for i in range(1, n):
        if order == 1 or (lower_order_final and i == n - 1):
            continue
        r = h[i - 1] / h[i]
        rows[i, 4], rows[i, 5] = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
    return rows


def dpm_solver_table(alphas_cumprod, S, skip_type="logSNR", order=2, lower_order_final=True):
    """(t_loop descending int64 [n], float32 table [n][DPM_ROW]) of the DPM-Solver++(2M) loop: dpm_solver_grid's steps, dpm_solver_rows'
    coefficients, everything in float64 and rounded to float32 once."""
    if order not in (1, 2):
        raise ValueError(f"order = {order!r}: the multistep solver is built for order 1 and 2")
    t_loop, ac_cur, ac_next = dpm_solver_grid(alphas_cumprod, S, skip_type)
    return t_loop, dpm_solver_rows(ac_cur, ac_next, order, lower_order_final).astype(np.float32)


def sampler_coef_table(alphacums32, S, eta, plms=False):
    """float32 table [n_steps][COEF_ROW] in LOOP order (row i = i-th executed step, index = n-1-i) plus
    the DDPM timestep of every row.  PLMS rows carry the Adams-Bashforth weights of plms.py:285-301."""
    ts = make_ddim_timesteps("uniform", S, len(alphacums32))
    sig, al, alp = make_ddim_sampling_parameters(alphacums32, ts, eta)
    sq1m = np.sqrt((np.float32(1.0) - al).astype(np.float32))
    n = ts.shape[0]
    tab = np.zeros((n, COEF_ROW), dtype=np.float32)
    for i in range(n):
        idx = n - 1 - i
        tab[i, 0:4] = [np.float32(al[idx]), np.float32(alp[idx]), np.float32(sig[idx]), sq1m[idx]]
        if plms:
            k = min(i, 3)
            ab = {0: ([1, 1, 0, 0], 2), 1: ([3, -1, 0, 0], 2), 2: ([23, -16, 5, 0], 12), 3: ([55, -59, 37, -9], 24)}[k]
            tab[i, 4:8] = ab[0]
            tab[i, 8] = ab[1]
        else:
            tab[i, 4:9] = [1, 0, 0, 0, 1]
    return tab, np.flip(ts).copy()
