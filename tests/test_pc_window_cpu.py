"""Host side of the batched PC extraction (main_pc_extract_inv --timestep_group, pc_drift.get_eigenvectors_window,
EditEngine.pc_window, AED_OP_PC_PROBE / _JACOBIAN / _ORTHONORMALISE): the Householder sign rule of the fp64 restatement
against torch.linalg.qr, the grouped control flow on stub functions, the refusals, and the window loop on the tape
interpreter against the oracle's per-timestep power iteration.  No GPU needed."""
import ctypes
import os
import re
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import pc_window_reference as ref
from audioeditingcode_amd import _lib as L
from audioeditingcode_amd import main_pc_extract_inv as pext
from audioeditingcode_amd import models, pc_drift
from audioeditingcode_amd.editing import Conditioning, EditEngine
from audioeditingcode_amd.scheduler import DDIMScheduler
from audioeditingcode_amd.tape import Tape
from audioeditingcode_amd.utils import PromptEmbeddings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the Householder rule
def _qr_cases():
    g = torch.Generator().manual_seed(11)
    rnd = lambda n, k: torch.randn(k, n, generator=g, dtype=torch.float64)                         # noqa: E731
    head = rnd(4096, 4)
    head[:, :600] = 0.0                               # a masked head: every pivot is a zero
    neg = head.clone()
    neg[1, :600] = -0.0                               # (jd / len) * mask leaves -0.0 where jd < 0
    neg[3, :600] = -0.0
    return [("random 4096 x 4", rnd(4096, 4), True), ("random 4096 x 8", rnd(4096, 8), True),
            ("random 4097 x 4", rnd(4097, 4), True), ("head rows zero", head, False), ("head rows -0.0 in two columns", neg, False)]


@pytest.mark.parametrize("name, dirs, random", _qr_cases(), ids=[c[0] for c in _qr_cases()])
def test_householder_rule_reproduces_lapack_signs(name, dirs, random):
    """pc_window_reference.orthonormal_rows against torch.linalg.qr in fp64 with the reference's sign and normalise rule
    (pc_drift._orthonormal_rows), SIGNS INCLUDED, to 1e-12.  For the random cases no pivot may be so small that rounding
    decides a sign; in the masked ones every pivot is a signed zero and the rule decides."""
    want = pc_drift._orthonormal_rows(dirs)
    got, margin = ref.orthonormal_rows(dirs.numpy())
    if random:
        assert margin >= 1e-3, margin
    else:
        assert margin == 0.0
        assert torch.signbit(dirs[1, :600]).all() == (name != "head rows zero")
    err = np.abs(got - want.numpy()).max()
    assert err < 1e-12, (name, err, margin)
    gram = got @ got.T
    assert np.abs(gram - np.eye(len(got))).max() < 1e-12


def test_restated_ops_sort_stably_and_keep_the_unsorted_lengths():
    g = np.random.default_rng(0)
    G, k, N = 2, 3, 64
    jd = g.standard_normal((G, k, N))
    jd[:, 2] *= 3.0
    jd[:, 1] = jd[:, 0] * np.sign(g.standard_normal(N))       # the same length as direction 0, bit for bit
    mask = np.ones(N)
    tab = np.tile(np.array([[0.5, 0.6, 0.8, 2.0]]), (G, 1))
    r = ref.pc_orthonormalise(jd, mask, np.zeros_like(jd), tab, 1e-3, 20)
    assert (r["lengths"][:, 0] == r["lengths"][:, 1]).all() and (r["lengths"][:, 2] > r["lengths"][:, 0]).all()
    for s in range(G):
        q, _ = ref.orthonormal_rows(jd[s] / r["lengths"][s][:, None])
        assert np.array_equal(r["unit"][s], q[[2, 0, 1]])       # descending, the tie in its original order
    assert r["in_corr"].shape == (G, k) and np.array_equal(r["snapshot"][1], r["lengths"] * 2.0)
    assert ref.pc_orthonormalise(jd, mask, np.zeros_like(jd), tab, 1e-3, 0)["in_corr"] is None
    assert ref.pc_orthonormalise(jd, mask, np.zeros_like(jd), tab, 1e-3, 10)["snapshot"] is None


# ------------------------------------------------------------------------------------------------ host logic on stubs
def _stub(T):
    """A deterministic model and function set: the eigenvectors of timestep t depend on t alone, and their sign alternates
    along the trajectory so the continuity rule has flips to make."""
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    model = SimpleNamespace(model=SimpleNamespace(scheduler=sched), kind="audioldm2", double_precision=False)
    calls = dict(single=[], window=[])

    def vectors(t, n_ev, shape):
        g = torch.Generator().manual_seed(int(t))
        q, _ = torch.linalg.qr(torch.randn(int(np.prod(shape)), n_ev, generator=torch.Generator().manual_seed(7)))
        sign = -1.0 if (int(t) // 10) % 2 else 1.0
        ev = (sign * q.T + 0.01 * torch.randn(n_ev, int(np.prod(shape)), generator=g)).reshape(n_ev, *shape)
        return ev, torch.arange(n_ev, 0, -1).float() * (1 + int(t) / 1000), [torch.full((n_ev,), 0.9)], \
            [torch.full((n_ev,), float(t))], {20: ev * 0.5}, {20: torch.ones(n_ev)}

    def get_eigenvectors(w, xt, text, uncond, latent, mask, t, x0_pred, pc_mode, const, cfg_tar, iters, dp, eta, n_ev):
        calls["single"].append(int(t))
        return vectors(t, n_ev, xt.shape[1:])

    def get_eigenvectors_window(w, xts, text, uncond, mask, ts, x0_preds, pc_mode, const, cfg_tar, iters, eta, n_ev):
        calls["window"].append([int(t) for t in ts])
        assert len(xts) == len(x0_preds) == len(ts)
        return [vectors(t, n_ev, x.shape[1:]) for t, x in zip(ts, xts)]

    def forward_directional(w, xt, t, latent, uncond, text, cfg_tar, eta=1, double_precision=False):
        return 0.9 * xt + 0.1 * latent, 0.5 * xt

    def inversion_forward_process(w, x0, etas=None, prompts=None, cfg_scales=None, prog_bar=False, num_inference_steps=50,
                                  numerical_fix=False):
        g = torch.Generator().manual_seed(2)
        return None, torch.randn(T, *x0.shape[1:], generator=g), torch.randn(T + 1, *x0.shape[1:], generator=g), None
    fns = SimpleNamespace(get_text_embeddings=lambda tp, tn, w: (None, "text", "uncond"), forward_directional=forward_directional,
                          inversion_forward_process=inversion_forward_process, get_eigenvectors=get_eigenvectors,
                          get_eigenvectors_window=get_eigenvectors_window, PCStreamChoice=pc_drift.PCStreamChoice)
    return model, fns, calls


def _args(T, **kw):
    a = Namespace(seed=5, cfg_tar=3, model_id="fake/fake", init_aud=None, num_diffusion_steps=T, source_prompt=["x"],
                  target_neg_prompt=[""], corr_to_swap=0.8, drift_start=9, drift_end=2, results_path="unused", const=1e-3,
                  n_evs=2, patch=[1, 3], iters=4, dry=False)
    a = pext.finish_args(a)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if torch.is_tensor(a):
        return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)
    return a == b


def test_timestep_group_gives_the_checkpoint_of_group_1_on_a_stub():
    T = 12                                            # window 9 -> 2: 7 steps; group 3 -> groups of 3, 3 and 1
    w0 = torch.randn(1, 2, 4, 3, generator=torch.Generator().manual_seed(1))
    model, fns, calls1 = _stub(T)
    a1 = _args(T)
    assert not hasattr(a1, "timestep_group")          # an args object from before the flag: getattr default 1
    cb1 = []
    ck1 = pext.extract_pcs(model, w0, a1, fns=fns, checkpoint_cb=lambda st: cb1.append(len(st["eigdata"])))
    assert len(calls1["single"]) == 7 and not calls1["window"] and cb1 == [0, 7]          # it = 0 and it = 10, as before
    model, fns, calls3 = _stub(T)
    cb3 = []
    ck3 = pext.extract_pcs(model, w0, _args(T, timestep_group=3), fns=fns, checkpoint_cb=lambda st: cb3.append(len(st["eigdata"])))
    ts = [int(t) for t in model.model.scheduler.timesteps]
    assert not calls3["single"] and calls3["window"] == [ts[3:6], ts[6:9], ts[9:10]]
    assert cb3 == [3, 6, 7]                           # once per finished group
    assert list(ck1) == list(ck3)
    for key in ("eigdata", "corrs", "in_corrs", "in_norms", "latents", "xts", "final"):
        assert _same(ck1[key], ck3[key]), key
    flips = torch.stack(ck3["corrs"])
    assert len(ck3["corrs"]) == 6 and (flips > 0).all()                                   # the rule flipped what pointed back
    raw = [fns.get_eigenvectors(None, w0, 0, 0, 0, 0, t, 0, 0, 0, 0, 0, 0, 0, 2)[0] for t in ts[3:10]]
    stored = [ck3["eigdata"][t]["eigvec"] for t in ts[3:10]]
    assert any(torch.equal(s, -r) for s, r in zip(stored, raw)) and torch.equal(stored[0], raw[0])
    # a group larger than the window is one call; dry runs and group 1 never call the window function
    model, fns, calls = _stub(T)
    pext.extract_pcs(model, w0, _args(T, timestep_group=16), fns=fns)
    assert calls["window"] == [ts[3:10]]
    model, fns, calls = _stub(T)
    pext.extract_pcs(model, w0, _args(T, timestep_group=4, dry=True), fns=fns)
    assert not calls["window"] and not calls["single"]


def test_cli_flag_and_refusals(capsys):
    assert pext.build_parser().parse_args([]).timestep_group == 1
    assert pext.build_parser().parse_args(["--timestep_group", "8"]).timestep_group == 8
    with pytest.raises(SystemExit):
        pext.main(["--timestep_group", "0"])
    assert "--timestep_group 0 < 1" in capsys.readouterr().err
    T = 12
    w0 = torch.zeros(1, 2, 4, 3)
    model, fns, _ = _stub(T)
    with pytest.raises(ValueError, match="timestep_group 0 < 1"):
        pext.extract_pcs(model, w0, _args(T, timestep_group=0), fns=fns)
    with pytest.raises(NotImplementedError, match="double_precision=True: the native path is fp32"):
        pext.extract_pcs(model, w0, _args(T, timestep_group=2, double_precision=True), fns=fns)
    model.kind = "stable_audio"
    with pytest.raises(NotImplementedError, match="Stable Audio is not supported"):
        pext.extract_pcs(model, w0, _args(T, timestep_group=2), fns=fns)
    emb = PromptEmbeddings(embedding_hidden_states=None, boolean_prompt_mask=None, embedding_class_lables=None)
    x = [torch.zeros(1, 2, 4, 3)]
    with pytest.raises(NotImplementedError, match="Stable Audio is not supported"):
        pc_drift.get_eigenvectors_window(model, x, emb, emb, torch.ones(1, 2, 4, 3), [1], x)
    model.kind, model.double_precision = "audioldm2", True
    with pytest.raises(NotImplementedError, match="double_precision=True"):
        pc_drift.get_eigenvectors_window(model, x, emb, emb, torch.ones(1, 2, 4, 3), [1], x)
    model.double_precision = False
    with pytest.raises(ValueError, match="1 xts and 1 x0_preds for 2 timesteps"):
        pc_drift.get_eigenvectors_window(model, x, emb, emb, torch.ones(1, 2, 4, 3), [1, 2], x)


def test_engine_refusals():
    T, C, H, W = 10, 8, 4, 2
    sched = DDIMScheduler()
    sched.set_timesteps(T)
    eng = EditEngine.__new__(EditEngine)
    eng.kind, eng.sched, eng.H, eng.W, eng.C = "audioldm2", sched, H, W, C
    cond = Conditioning(ehs0=torch.zeros(1, 8, 4), ehs1=torch.zeros(1, 3, 6), mask1=torch.ones(1, 3))
    ts = [int(t) for t in sched.timesteps[2:4]]
    x, mask = torch.zeros(2, C, H, W), torch.ones(C, H, W)

    def run(xts=x, x0=x, mask=mask, ts=ts, text=cond, init=torch.zeros(2, 2, C, H, W), toe=torch.ones(2), **kw):
        return eng.pc_window(xts, x0, mask, ts, text, cond, init, toe, **kw)
    with pytest.raises(ValueError, match="0 timesteps"):
        run(ts=[])
    with pytest.raises(ValueError, match="0 iterations"):
        run(iters=0)
    with pytest.raises(ValueError, match=r"init \(2, 9, 8, 4, 2\), expected \[G = 2, n_ev <= 8"):
        run(init=torch.zeros(2, 9, C, H, W))
    with pytest.raises(ValueError, match="init"):
        run(init=torch.zeros(3, 2, C, H, W))
    with pytest.raises(ValueError, match="xts"):
        run(xts=torch.zeros(3, C, H, W))
    with pytest.raises(ValueError, match="x0_preds"):
        run(x0=torch.zeros(2, C, H, 3))
    with pytest.raises(ValueError, match="mask"):
        run(mask=torch.ones(1, H, W))
    with pytest.raises(ValueError, match="pc_mode 4"):
        run(pc_mode=4)
    with pytest.raises(ValueError, match="to_eigval"):
        run(toe=torch.ones(3))
    with pytest.raises(ValueError, match="2 / 1 rows, one each"):
        run(text=Conditioning(ehs0=torch.zeros(2, 8, 4), ehs1=torch.zeros(2, 3, 6), mask1=torch.ones(2, 3)))
    G = 20
    with pytest.raises(ValueError, match="320 U-Net rows, at most 256"):
        eng.pc_window(torch.zeros(G, C, H, W), torch.zeros(G, C, H, W), mask, [1] * G, cond, cond,
                      torch.zeros(G, 8, C, H, W), torch.ones(G))
    eng.kind = "stable_audio"
    with pytest.raises(ValueError, match="not supported"):
        run()


# ------------------------------------------------------------------------------------------------ the library and the tape
def test_library_takes_the_three_opcodes():
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "aed.h")).read()
    for name, code in (("PC_PROBE", 31), ("PC_JACOBIAN", 32), ("PC_ORTHONORMALISE", 33)):
        assert re.search(rf"AED_OP_{name}\s*=\s*{code}\b", hdr) and getattr(L, "OP_" + name) == code
    lib = L.lib()
    t = torch.zeros(64)
    ti = torch.zeros(4, dtype=torch.int32)
    tp = Tape("cpu")
    tp.pc_probe(x_in=t, xt=t, probe=t, tab=t, G=1, k=2, C=2, HW=4, mode=3)
    tp.pc_jacobian(eps=t, xt=t, probe=t, tab=t, x0_pred=t, mask=t, jd=t, G=1, k=2, C=2, HW=4, cfg=3.0, v_pred=1)
    tp.pc_orthonormalise(jd=t, mask=t, unit=t, previous=t, probe=t, state=ti, stats=t, tab=t, G=1, k=9, N=8, iters=5,
                         const=1e-2, snap_vec=t, snap_val=t, S=1)
    assert [m["name"] for m in tp.meta] == ["pc_probe", "pc_jacobian", "pc_orthonormalise"]
    probe, jac, orth = tp.ops
    assert probe.code == 31 and list(probe.i[:5]) == [1, 2, 2, 4, 3] and probe.p[3] == t.data_ptr()
    assert jac.code == 32 and list(jac.i[:5]) == [1, 2, 2, 4, 1] and jac.f[0] == 3.0 and jac.p[6] == t.data_ptr()
    assert orth.code == 33 and list(orth.i[:6]) == [1, 9, 8, 5, 1, 0] and abs(orth.f[0] - 1e-2) < 1e-9
    assert orth.p[5] == ti.data_ptr() and orth.p[9] == t.data_ptr()
    # refused before anything is launched
    assert lib.aed_launch(ctypes.byref(orth), None) != 0
    assert b"9 directions, at most 8" in lib.aed_last_error()
    probe.i[4] = 0
    assert lib.aed_launch(ctypes.byref(probe), None) != 0 and b"pc_mode 0" in lib.aed_last_error()
    jac.p[5] = None
    assert lib.aed_launch(ctypes.byref(jac), None) != 0 and b"null pointer in slot p5" in lib.aed_last_error()


# ------------------------------------------------------------------------------------------------ the loop on CPU
def test_window_loop_on_cpu_matches_the_oracle_per_timestep(monkeypatch):
    """tiny/audioldm2, T = 10, latent 8x32x16, two consecutive timesteps x n_ev 2 x 3 iterations in one pc_window loop on the
    tape interpreter (the three ops restated by pc_window_reference) against oracle.pc.get_eigenvectors run per timestep from
    the same start vectors: the thresholds of test_gpu_pc.test_power_iteration_and_drift_match_oracle."""
    from conftest import install_cpu_stack
    from oracle import loops as oloops, pc as opc, tape_interp, unet as ounet
    from oracle.scheduler import OracleDDIMScheduler
    install_cpu_stack(monkeypatch)
    for code, fn in ((L.OP_PC_PROBE, ref.interp_probe), (L.OP_PC_JACOBIAN, ref.interp_jacobian),
                     (L.OP_PC_ORTHONORMALISE, ref.interp_orthonormalise)):
        monkeypatch.setitem(tape_interp.DISPATCH, code, fn)
    T, n_ev, iters, shape = 10, 2, 3, (8, 32, 16)

    class _Cpu(models.AudioLDM2Wrapper):
        def _require_device(self):
            pass
    m = _Cpu(model_id="tiny/audioldm2", device="cpu", seed=0)
    m.load_scheduler()
    m.model.scheduler.set_timesteps(T, device=None)
    cfg, sd = m.family["unet"], m.state_dicts["unet"]
    osched = OracleDDIMScheduler()
    osched.set_timesteps(T)

    def unet_fn(x, t, cond):
        hs, cl, mk = (v.cpu() for v in cond)
        ex = lambda v: v if v.shape[0] == x.shape[0] else v.expand(x.shape[0], *v.shape[1:])      # noqa: E731
        return ounet.unet_forward(cfg, sd, x, t, encoder_hidden_states=ex(hs), encoder_hidden_states_1=ex(cl),
                                  encoder_attention_mask_1=ex(mk))[0]
    ow = oloops.OracleWrapper(osched, unet_fn)
    g = torch.Generator().manual_seed(3)
    ts = m.model.scheduler.timesteps[4:6]
    xts = [torch.randn(1, *shape, generator=g) * 0.8 for _ in ts]
    latent = torch.randn(1, *shape, generator=g)
    inits = [torch.randn(n_ev, *shape, generator=g) for _ in ts]
    mask = torch.zeros(1, *shape)
    mask[:, :, 6:26, :] = 1                           # --patch 6 26: the head rows are masked
    emb = lambda p: PromptEmbeddings(embedding_hidden_states=m.encode_text(p)[0], embedding_class_lables=m.encode_text(p)[1],   # noqa: E731
                                     boolean_prompt_mask=m.encode_text(p)[2])
    c_unc, c_txt = m.encode_text([""]), m.encode_text(["a dog barking"])
    x0s = [opc.forward_directional(ow, x, t, latent, c_unc, c_txt, 3.0, eta=1.0)[1] for x, t in zip(xts, ts)]
    got = pc_drift.get_eigenvectors_window(m, xts, emb(["a dog barking"]), emb([""]), mask, ts, x0s, pc_drift.PCStreamChoice.BOTH,
                                           1e-2, 3.0, iters, 1.0, n_ev, init_eigvecs=inits)
    assert len(got) == 2
    rep = lambda c: tuple(v.repeat(n_ev, *[1] * (v.dim() - 1)) for v in c)                        # noqa: E731
    for j, t in enumerate(ts):
        ev, val, in_corr, in_norm, iv, il = got[j]
        ev_o, val_o, corr_o, nrm_o = opc.get_eigenvectors(ow, xts[j], rep(c_txt), rep(c_unc), latent, mask, t, x0s[j], inits[j],
                                                          const=1e-2, cfg_tar=3.0, iters=iters, eta=1.0, n_ev=n_ev)
        assert ev.shape == (n_ev, *shape) and val.shape == (n_ev,) and len(in_corr) == iters - 1 and len(in_norm) == iters
        assert iv == {} and il == {}
        gram = ev.reshape(n_ev, -1) @ ev.reshape(n_ev, -1).T
        assert (gram - torch.eye(n_ev)).abs().max() < 1e-4
        torch.testing.assert_close(val.reshape(-1), torch.as_tensor(val_o).reshape(-1), rtol=5e-2, atol=1e-6)
        cos = (ev.reshape(n_ev, -1) * ev_o.reshape(n_ev, -1)).sum(1)
        assert cos.abs().min() > 0.99, (j, cos)
        assert (cos > 0).all(), (j, cos)              # the masked head: LAPACK's sign for a zero pivot
        for a, b in zip(in_norm, nrm_o):
            torch.testing.assert_close(a, b, rtol=5e-2, atol=1e-7)
