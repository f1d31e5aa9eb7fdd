"""Host checks of tests/lstm_core_ref.py (no GPU): the fp64 reference of the LSTM recurrent core must not be its own only witness.  The free-running
forms are held to torch.nn.LSTM and torch.autograd in fp64, the per-step form to the free-running one, and elem_err with the GPU tests' bounds is
shown to flag planted single-element errors that the whole-tensor relative L2 of tests/test_gpu_lstm.py lets through."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lstm_core_ref as R      # noqa: E402

H, G = R.H, R.G


def _nn_lstm(w, ndir):
    """torch.nn.LSTM in fp64 that is fed a given xproj: the input is the directions' xproj rows side by side, weight_ih picks direction d's block"""
    m = torch.nn.LSTM(input_size=ndir * G, hidden_size=H, batch_first=True, bidirectional=ndir == 2).double()
    with torch.no_grad():
        for d, sfx in enumerate(['', '_reverse'][:ndir]):
            wi = torch.zeros(G, ndir * G, dtype=torch.float64)
            wi[:, d * G:(d + 1) * G] = torch.eye(G, dtype=torch.float64)
            getattr(m, 'weight_ih_l0' + sfx).copy_(wi)
            getattr(m, 'weight_hh_l0' + sfx).copy_(w[d].double())
            getattr(m, 'bias_ih_l0' + sfx).zero_()
            getattr(m, 'bias_hh_l0' + sfx).zero_()
    return m


def _nn_input(xproj, B, T, ndir):
    return xproj.double().permute(1, 2, 0, 3).reshape(B, T, ndir * G).clone().requires_grad_(True)


@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('ndir', [1, 2])
def test_free_running_forms_vs_torch_lstm_and_autograd(T, ndir):
    B = 2
    w, xproj, dh = R.random_operands(B, T, ndir, 10 * T + ndir)
    gates, c, h = R.lstm_fwd_free(w, xproj, B, T, ndir, round_h=False)
    x = _nn_input(xproj, B, T, ndir)
    rh, _ = _nn_lstm(w, ndir)(x)
    assert (h - rh).abs().max().item() < 1e-10
    gx, = torch.autograd.grad((rh * dh.double()).sum(), x)
    want = gx.reshape(B, T, ndir, G).permute(2, 0, 1, 3)
    for ld, pad in ((ndir * H, 0), (ndir * H + 8, 8)):           # the padded leading dimension reads the same columns
        dhp = torch.cat([dh, torch.full((B, T, pad), float('nan'))], dim=-1)
        dg = R.lstm_bwd_ref(w, gates, c, dhp, ld, B, T, ndir)
        assert (dg - want).abs().max().item() < 1e-10
    # c_{-1} = 0: the forget gate's gradient at the sequence start is exactly zero
    assert torch.count_nonzero(dg[0, :, 0, H:2 * H]) == 0 and (T == 1 or torch.count_nonzero(dg[0, :, 1, H:2 * H]) > 0)
    if ndir == 2:
        assert torch.count_nonzero(dg[1, :, T - 1, H:2 * H]) == 0 and torch.count_nonzero(want[1, :, T - 1, H:2 * H]) == 0


@pytest.mark.parametrize('B,T,ndir', [(1, 1, 1), (2, 3, 2), (2, 7, 2)])
def test_step_form_reproduces_the_free_running_one(B, T, ndir):
    """fed the free-running reference's own rounded h and its c, the per-step form returns the same gates, c and (before rounding) h; the
    teacher-forced backward fed the free-running dgates returns them"""
    w, xproj, dh = R.random_operands(B, T, ndir, 77 + T)
    gates, c, h = R.lstm_fwd_free(w, xproj, B, T, ndir)
    sg, sc, sh = R.lstm_fwd_step_ref(w, xproj, h.bfloat16(), c, B, T, ndir)
    assert (sg - gates).abs().max().item() < 1e-13 and (sc - c).abs().max().item() < 1e-13
    assert torch.equal(R.bf16_round(sh), R.h_by_dir(h, B, T, ndir))
    free = R.lstm_bwd_ref(w, gates, c, dh, ndir * H, B, T, ndir)
    assert (R.lstm_bwd_ref(w, gates, c, dh, ndir * H, B, T, ndir, dgates_kernel=free) - free).abs().max().item() < 1e-13
    # the judges pass what the reference itself produces (fp32 c and gates, bf16 h and dgates, as a kernel returns them)
    for name, (v, where, bound) in R.judge_forward(w, xproj, h.bfloat16(), gates.float(), c.float(), B, T, ndir).items():
        assert v < bound, (name, v, where)
    fr = R.lstm_bwd_ref(w, gates.float(), c.float(), dh, ndir * H, B, T, ndir, round_dg=True)
    v, where, bound = R.judge_backward(w, gates.float(), c.float(), dh, ndir * H, fr.bfloat16(), B, T, ndir)
    assert v < bound, (v, where)


def _outputs(B, T, ndir, seed):
    w, xproj, dh = R.random_operands(B, T, ndir, seed)
    gates, c, h = R.lstm_fwd_free(w, xproj, B, T, ndir)
    gates, c, h = gates.float(), c.float(), h.bfloat16()
    dg = R.lstm_bwd_ref(w, gates, c, dh, ndir * H, B, T, ndir, round_dg=True).bfloat16()
    return w, xproj, dh, gates, c, h, dg


def _flagged(res, name, where=None):
    v, at, bound = res[name] if isinstance(res, dict) else res
    return v >= bound and (where is None or tuple(at[:len(where)]) == tuple(where))


def test_planted_errors_are_flagged_per_element():
    B, T, ndir, t0 = 2, 9, 2, 5
    w, xproj, dh, gates, c, h, dg = _outputs(B, T, ndir, 5)
    fwd = lambda hh, gg, cc: R.judge_forward(w, xproj, hh, gg, cc, B, T, ndir)      # noqa: E731
    clean = fwd(h, gates, c)
    assert all(v < bound for v, _, bound in clean.values()), clean
    # one unit of one gate at one step off by 1e-3
    bad = gates.clone()
    bad[1, 1, t0, 2 * H + 77] += 1e-3
    assert _flagged(fwd(h, bad, c), 'gates', (1, 1, t0, 2, 77))
    # one step's xproj row replaced by the row three steps earlier: what a kernel that read a stale ring row would return
    xs = xproj.clone()
    xs[0, 1, t0] = xproj[0, 1, t0 - 3]
    sg, sc, sh = R.lstm_fwd_free(w, xs, B, T, ndir)
    res = fwd(sh.bfloat16(), sg.float(), sc.float())
    assert _flagged(res, 'gates', (0, 1, t0)) and _flagged(res, 'c', (0, 1, t0)) and _flagged(res, 'h', (0, 1, t0))
    # c reset to 0 at one step
    bad = c.clone()
    bad[0, 0, t0] = 0
    assert _flagged(fwd(h, gates, bad), 'c', (0, 0, t0))
    # four bf16 ulps on one h
    bad = h.clone()
    u = int(h[1, t0, H:].float().abs().argmax())
    bad.view(torch.int16)[1, t0, H + u] += 4
    assert _flagged(fwd(bad, gates, c), 'h', (1, 1, t0, None, u))
    # one dgates element scaled by 1.02
    bwd = lambda x: R.judge_backward(w, gates, c, dh, ndir * H, x, B, T, ndir)      # noqa: E731
    assert bwd(dg)[0] < R.DGATE_BOUND
    j = int(dg[1, 0, t0].float().abs().argmax())
    bad = dg.double().clone()
    bad[1, 0, t0, j] *= 1.02
    assert _flagged(bwd(bad), None, (1, 0, t0, j // H, j % H))


def test_whole_tensor_l2_misses_single_step_errors_at_bench_length():
    """at T = 1001 the relative L2 of tests/test_gpu_lstm.py (1.5e-2) passes every single-element plant that elem_err flags"""
    B, T, ndir, t0 = 1, 1001, 1, 500
    w, xproj, dh, gates, c, h, dg = _outputs(B, T, ndir, 6)
    rg, rc, rh = R.lstm_fwd_step_ref(w, xproj, h, c, B, T, ndir)
    hd = R.h_by_dir(h, B, T, ndir)
    plants = []
    bad = gates.clone()
    bad[0, 0, t0, 3 * H + 5] += 1e-3
    plants.append(('gates', bad, rg, R.elem_err(bad, rg)[0] >= R.GATE_BOUND))
    bad = gates.clone()                                     # a stale xproj row at one step, seen in that step's gates
    bad[0, 0, t0] = R.lstm_fwd_step_ref(w, xproj.roll(3, dims=2), h, c, B, T, ndir)[0][0, 0, t0].float()
    plants.append(('stale row', bad, rg, R.elem_err(bad, rg)[0] >= R.GATE_BOUND))
    bad = c.clone()
    bad[0, 0, t0] = 0
    plants.append(('c reset', bad, rc, R.elem_err(bad, rc, rel=R.C_REL)[0] >= R.C_BOUND))
    bad = hd.clone().contiguous()
    bad.view(torch.int16)[0, 0, t0, int(hd[0, 0, t0].float().abs().argmax())] += 4
    plants.append(('h ulps', bad, rh, R.elem_err(bad, rh, rel=R.BF16_REL)[0] >= R.H_BOUND))
    rd = R.lstm_bwd_ref(w, gates, c, dh, H, B, T, ndir, dgates_kernel=dg)
    bad = dg.double().clone()
    bad[0, 0, t0, int(dg[0, 0, t0].float().abs().argmax())] *= 1.02
    plants.append(('dgates', bad, rd, R.elem_err(bad, rd, rel=R.BF16_REL, floor=R.dh_scale(dh, H, B, T, ndir))[0] >= R.DGATE_BOUND))
    for name, bad, ref, seen in plants:
        assert seen, name
        # a whole wrong row out of 1001 is 1 / sqrt(1001) = 3.2e-2 of the tensor: over the 1.5e-2 of the outputs, under the 4e-2 which that file
        # allows the parameter gradients, the only place where it sees the recurrent core's backward
        assert R.rel_l2(bad, ref) < (4e-2 if name in ('stale row', 'c reset') else 1.5e-2), (name, R.rel_l2(bad, ref))
