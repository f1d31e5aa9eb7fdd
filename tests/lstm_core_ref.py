"""Float64 reference for the recurrent core of the (Bi)LSTM heads (csrc/lstm.hip: se_lstm_fwd_bf16 / se_lstm_bwd_bf16) in the C ABI's layouts,
and the per-element error metric of its parity tests.  Test infrastructure only: torch on the CPU, no kernel.

    w_hh [ndir][1024][256] (gate order i, f, g, o)    xproj, gates [ndir][B][T][1024]    c [ndir][B][T][256]    h, dh_out (B, T, ndir * 256 [+ pad])
    pre = W_hh h_prev + xproj[t]    i, f, o = sigmoid(pre)    g = tanh(pre)    c = f c_prev + i g    h = o tanh(c)    (direction 1 runs t = T-1 .. 0)

A free-running fp64 LSTM drifts from the kernel, which rounds h to bf16 every step, so the kernels are judged STEP BY STEP on their own inputs:
lstm_fwd_step_ref takes the kernel's h_out / c_out of the previous step as the state, lstm_bwd_ref the kernel's dgates of the previously processed
step as the source of the recurrent dh; by induction from the zero state every step right on its own inputs means the sequence is right.
tests/test_lstm_core_ref_host.py holds these forms to torch.nn.LSTM and torch.autograd and shows that elem_err with the bounds below sees planted
single-element errors; tests/test_gpu_lstm_core.py compares the kernels with them."""
import torch

H, G = 256, 1024

# ---- bounds of tests/test_gpu_lstm_core.py, shared with the planted-error test --------------------------------------------------------------
# Ceilings, from the arithmetic: a gate is the fp32 MFMA sum of 256 bf16 x bf16 products (|pre| <= 16) through v_exp_f32 and v_rcp_f32 at 1 ulp
# each; the argument scaling of __expf has relative error 2^-24 |x| log2(e): below 4e-6 absolute.  c adds its own fp32 rounding (2^-22 |c|), h and
# dgates are rounded to bf16 (2^-8 relative covers round-to-nearest of a value that carries fp32 error).  dgates: products of at most five fp32
# factors, each <= 1 except dh / dc: 1e-5 of max(1, max |dh_out row|).
GATE_CEILING, DGATE_CEILING = 4e-6, 1e-5
C_REL, BF16_REL = 2.0 ** -22, 2.0 ** -8
# Asserted bounds: ~2x the worst value measured on the MI355X over the cases of test_gpu_lstm_core.py (conftest.bounded keeps the log), never above
# the ceilings.  The kernels and the seeded operands are deterministic, so the measured figures repeat exactly.  Measured worst, all at
# (B, T, ndir) = (2, 1001, 2): gates 5.07e-7, c 3.37e-7 over 2^-22 |c|, h 6.9e-8 over 2^-8 |h|, dgates 1.49e-8 over 2^-8 |dgates| (round-to-nearest
# stays inside 2^-8, so what is left over it shows only where the reference is next to zero).
GATE_BOUND = 1e-6                  # absolute, gates_out
C_BOUND = 7e-7                     # absolute part of c_out: |c - ref| <= C_BOUND + C_REL |ref|
H_BOUND = 1.5e-7                   # absolute part of h_out: |h - ref| <= H_BOUND + BF16_REL |ref|
DGATE_BOUND = 3e-8                 # absolute part of dgates_out over max(1, max |dh_out row|), on the kernel's own previous dgates
assert max(GATE_BOUND, C_BOUND, H_BOUND) <= GATE_CEILING and DGATE_BOUND <= DGATE_CEILING
# free-running comparison at T <= 7.  The reference rounds the dgates it feeds back to bf16 as the kernel does, so the two differ only where the
# kernel's fp32 value and the fp64 one fall on different sides of a rounding boundary: one bf16 ulp (2^-8 |dg_j|) on one of the 1024 fed-back
# elements, which moves dh_rec[k] by |W[j][k]| 2^-8 |dg_j|.  With |W| <= 0.6 (4.5 sigma of N(0, 1/64)) and |dg_j| <= 0.25 |dc|, three such flips
# of the largest weights in one sum stay below 2e-3 of the row scale.
DGATE_FREE_CEILING = 2e-3
DGATE_FREE_BOUND = 8e-5            # measured worst 3.97e-5 at (1, 6, 2); 0 to 1.9e-5 at the other shapes with T <= 7


def random_operands(B, T, ndir, seed):
    """W_hh ~ N(0, 1/64) as bf16 (the recurrent term is comparable with xproj), xproj ~ 1.5 N(0, 1) fp32, dh_out ~ N(0, 1) fp32 (B, T, ndir 256)"""
    gen = torch.Generator().manual_seed(seed)
    w = (torch.randn(ndir, G, H, generator=gen) / 8.0).bfloat16()
    xproj = torch.randn(ndir, B, T, G, generator=gen) * 1.5
    dh = torch.randn(B, T, ndir * H, generator=gen)
    return w, xproj, dh


def bf16_round(x):
    return x.float().bfloat16().double()


def _from(x, d, earlier):
    """x (B, T, n) -> the value at the step the forward of direction d visited just before (earlier) or just after each t, zero where there is none"""
    out = torch.zeros_like(x)
    if (d == 0) == earlier:
        out[:, 1:] = x[:, :-1]
    else:
        out[:, :-1] = x[:, 1:]
    return out


def h_by_dir(h, B, T, ndir):
    """(B, T, ndir * 256) or (B * T, ndir * 256) -> [ndir][B][T][256]"""
    return h.reshape(B, T, ndir, H).permute(2, 0, 1, 3)


def _cell(pre, c_prev):
    i, f, g, o = pre.split(H, dim=-1)
    i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
    c = f * c_prev + i * g
    return torch.cat([i, f, g, o], dim=-1), c, o * torch.tanh(c)


def lstm_fwd_free(w_hh, xproj, B, T, ndir, round_h=True):
    """the plain recurrence; h is rounded to bf16 between steps (and in the returned tensor) unless round_h is False.
    Returns gates [ndir][B][T][1024], c [ndir][B][T][256], h (B, T, ndir * 256), all fp64"""
    W, x = w_hh.double(), xproj.double().reshape(ndir, B, T, G)
    gates, c_all = torch.zeros(ndir, B, T, G, dtype=torch.float64), torch.zeros(ndir, B, T, H, dtype=torch.float64)
    h_all = torch.zeros(B, T, ndir * H, dtype=torch.float64)
    for d in range(ndir):
        h, c = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        for s in range(T):
            t = T - 1 - s if d == 1 else s
            gates[d, :, t], c, h = _cell(h @ W[d].T + x[d, :, t], c)
            if round_h:
                h = bf16_round(h)
            c_all[d, :, t], h_all[:, t, d * H:(d + 1) * H] = c, h
    return gates, c_all, h_all


def lstm_fwd_step_ref(w_hh, xproj, h_kernel, c_kernel, B, T, ndir):
    """every step on the KERNEL's previous state: h_kernel (B, T, ndir * 256) bf16, c_kernel [ndir][B][T][256] fp32.
    Returns reference gates [ndir][B][T][1024], c and h [ndir][B][T][256] (h unrounded), fp64; one batched matmul per direction"""
    W, x = w_hh.double(), xproj.double().reshape(ndir, B, T, G)
    hk, ck = h_by_dir(h_kernel.double(), B, T, ndir), c_kernel.double().reshape(ndir, B, T, H)
    out = [_cell(_from(hk[d], d, True) @ W[d].T + x[d], _from(ck[d], d, True)) for d in range(ndir)]
    return tuple(torch.stack([o[k] for o in out]) for k in range(3))


def lstm_bwd_ref(w_hh, gates, c_saved, dh_out, ld_dh, B, T, ndir, dgates_kernel=None, round_dg=False):
    """d loss / d xproj [ndir][B][T][1024] (fp64, unrounded) of loss = sum(h . dh_out), from the saved post-activation gates and c.
    dgates_kernel None: free running (round_dg: the dgates fed back through W_hh^T are rounded to bf16 first, as the kernel's are).
    Otherwise the recurrent dh of every step is W_hh^T dgates_kernel[the step processed before it]; the cell gradient dc is carried in fp64."""
    W = w_hh.double()
    gt, cs = gates.double().reshape(ndir, B, T, G), c_saved.double().reshape(ndir, B, T, H)
    dh_all = dh_out.double().reshape(B, T, ld_dh)
    out = torch.zeros(ndir, B, T, G, dtype=torch.float64)
    for d in range(ndir):
        rec_all = None if dgates_kernel is None else _from(dgates_kernel.double().reshape(ndir, B, T, G)[d], d, False) @ W[d]
        c_prev = _from(cs[d], d, True)
        dh_rec, dc_rec = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
        for s in range(T):
            t = s if d == 1 else T - 1 - s                  # the forward visited t last-to-first in this order
            gi, gf, gg, go = gt[d, :, t].split(H, dim=-1)
            dh = dh_all[:, t, d * H:(d + 1) * H] + (dh_rec if rec_all is None else rec_all[:, t])
            tc = torch.tanh(cs[d, :, t])
            dc = dh * go * (1 - tc * tc) + dc_rec
            dg = torch.cat([dc * gg * gi * (1 - gi), dc * c_prev[:, t] * gf * (1 - gf), dc * gi * (1 - gg * gg), dh * tc * go * (1 - go)], dim=-1)
            out[d, :, t] = dg
            dc_rec = dc * gf
            dh_rec = (bf16_round(dg) if round_dg else dg) @ W[d]
    return out


def elem_err(got, ref, rel=0.0, floor=1.0):
    """worst excess of |got - ref| over rel |ref|, in units of `floor` (a number, or a tensor that broadcasts against ref: a per-row scale), and where:
    (value, (dir, b, t, gate, unit)) for tensors laid out [ndir][B][T][1024 or 256] (gate is None for the 256-wide c and h)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape and ref.dim() == 4, (got.shape, ref.shape)
    e = ((got - ref).abs() - rel * ref.abs()) / floor
    e = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)        # an unwritten (NaN) element is the worst possible
    k = int(e.argmax())
    d, r = divmod(k, ref[0].numel())
    b, r = divmod(r, ref[0, 0].numel())
    t, j = divmod(r, ref.shape[-1])
    return e.reshape(-1)[k].item(), (d, b, t, j // H if ref.shape[-1] == G else None, j % H)


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).norm() / ref.norm()).item()


def dh_scale(dh_out, ld_dh, B, T, ndir):
    """max(1, max |dh_out row|) per (dir, b, t) as [ndir][B][T][1]: the unit of the dgates floor"""
    rows = h_by_dir(dh_out.double().reshape(B, T, ld_dh)[..., :ndir * H].contiguous(), B, T, ndir)
    return rows.abs().amax(dim=-1, keepdim=True).clamp(min=1.0)


def judge_forward(w_hh, xproj, h, gates, c, B, T, ndir):
    """the forward's per-step parity: {name: (worst excess, (dir, b, t, gate, unit), bound)} of gates_out, c_out and h_out against the step reference"""
    rg, rc, rh = lstm_fwd_step_ref(w_hh, xproj, h, c, B, T, ndir)
    return {'gates': elem_err(gates.reshape(ndir, B, T, G), rg) + (GATE_BOUND,),
            'c': elem_err(c.reshape(ndir, B, T, H), rc, rel=C_REL) + (C_BOUND,),
            'h': elem_err(h_by_dir(h, B, T, ndir), rh, rel=BF16_REL) + (H_BOUND,)}


def judge_backward(w_hh, gates, c, dh_out, ld_dh, dgates, B, T, ndir):
    """the backward's per-step parity on the kernel's own previous dgates: (worst excess, where, bound)"""
    ref = lstm_bwd_ref(w_hh, gates, c, dh_out, ld_dh, B, T, ndir, dgates_kernel=dgates)
    return elem_err(dgates.reshape(ndir, B, T, G), ref, rel=BF16_REL, floor=dh_scale(dh_out, ld_dh, B, T, ndir)) + (DGATE_BOUND,)
