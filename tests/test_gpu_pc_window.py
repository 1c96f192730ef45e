"""The batched PC extraction on the GPU: the three kernels of csrc/pc.hip on raw buffers against the fp64 restatement
(tests/pc_window_reference.py) and fp32 torch, then pc_drift.get_eigenvectors_window / extract_pcs --timestep_group on
tiny/audioldm2 against the CPU oracle and against the per-timestep path."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pc_window_reference as ref                                          # noqa: E402
from audioeditingcode_amd import models, pc_drift                          # noqa: E402
from audioeditingcode_amd.tape import Tape                                 # noqa: E402
from audioeditingcode_amd.utils import PromptEmbeddings                    # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 5, 3), (8, 32, 16), (8, 33, 16)]          # N = 120 (less than one workgroup), 4096, 4224
KS, GS = (1, 2, 4, 8), (1, 3)


def _masks(C, H, W):
    ones = torch.ones(C, H, W)
    tail = ones.clone()
    tail[..., W - max(1, W // 4):] = 0                  # the mask of test_gpu_pc: the tail of the last dimension
    band = torch.zeros(C, H, W)
    band[:, max(1, H // 5):H - max(1, H // 5), :] = 1   # --patch: the head rows, and with them every pivot, are masked
    return dict(ones=ones, tail=tail, band=band)


def _tab(G, g):
    abar = torch.rand(G, generator=g) * 0.8 + 0.1
    return torch.stack([abar.sqrt(), (1 - abar).sqrt(), abar ** 0.5, (1 / abar - 1) / 1e-2], 1).contiguous()


# ------------------------------------------------------------------------------------------------ probe and jacobian
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_probe_and_jacobian_are_bit_equal_to_fp32_torch(shape):
    C, H, W = shape
    HW, N = H * W, C * H * W
    gen = torch.Generator().manual_seed(N)
    mask = _masks(C, H, W)["band"].reshape(N)
    for G in GS:
        for k in KS:
            xt, x0p = torch.randn(G, N, generator=gen), torch.randn(G, N, generator=gen)
            probe = torch.randn(G, k, N, generator=gen) * 1e-2
            eps = torch.randn(G, 2 * k, HW, C, generator=gen)
            tab = _tab(G, gen)
            d = {n: v.to(DEV) for n, v in dict(xt=xt, x0p=x0p, probe=probe, eps=eps, tab=tab, mask=mask).items()}
            moved = xt[:, None] + probe * tab[:, 0].reshape(G, 1, 1)                       # forward_directional's expression
            still = xt[:, None].expand_as(moved)
            for mode, cfg, v_pred in ((1, 3.0, 0), (2, 3.3, 1), (3, 1.0, 0)):
                x_in = torch.full((G, 2 * k, HW, C), float("nan"), device=DEV)
                jd = torch.full((G, k, N), float("nan"), device=DEV)
                tp = Tape(DEV)
                tp.pc_probe(x_in=x_in, xt=d["xt"], probe=d["probe"], tab=d["tab"], G=G, k=k, C=C, HW=HW, mode=mode)
                tp.pc_jacobian(eps=d["eps"], xt=d["xt"], probe=d["probe"], tab=d["tab"], x0_pred=d["x0p"], mask=d["mask"],
                               jd=jd, G=G, k=k, C=C, HW=HW, cfg=cfg, v_pred=v_pred)
                tp.run()
                rows = torch.cat([moved if mode != 2 else still, moved if mode != 3 else still], 1)
                want_x = rows.reshape(G, 2 * k, C, HW).transpose(2, 3).contiguous()
                e = eps.transpose(2, 3).reshape(G, 2 * k, N)
                e = e[:, :k] + cfg * (e[:, k:] - e[:, :k])
                c0, c1 = tab[:, 1].reshape(G, 1, 1), tab[:, 2].reshape(G, 1, 1)
                x0 = (moved - c0 * e) / c1 if not v_pred else c1 * moved - c0 * e
                want_jd = x0 * mask - x0p[:, None]
                assert torch.equal(x_in.cpu(), want_x), (shape, G, k, mode)
                assert torch.equal(jd.cpu(), want_jd), (shape, G, k, mode, v_pred)
                if mode == 1 and G == 1 and k == 2:      # the restatement the CPU loop runs is the same arithmetic
                    assert np.array_equal(ref.pc_probe(xt.numpy(), probe.numpy(), tab.numpy(), C, HW, mode, np.float32),
                                          want_x.numpy())
                    assert np.array_equal(ref.pc_jacobian(eps.numpy(), xt.numpy(), probe.numpy(), tab.numpy(), x0p.numpy(),
                                                          mask.numpy(), C, HW, cfg, bool(v_pred), np.float32), want_jd.numpy())


# ------------------------------------------------------------------------------------------------ orthonormalise
def _orthonormalise(jd, mask, previous, tab, const, it, iters=1, S=0, state=None):
    """One launch of the op on copies of the inputs.  Returns CPU tensors."""
    G, k, N = jd.shape
    d = dict(jd=jd.to(DEV).clone(), mask=mask.to(DEV), unit=torch.full((G, k, N), float("nan"), device=DEV),
             previous=previous.to(DEV).clone(), probe=torch.full((G, k, N), float("nan"), device=DEV),
             stats=torch.zeros(2, iters, G, k, device=DEV), tab=tab.to(DEV),
             snap_vec=torch.zeros(max(S, 1), G, k, N, device=DEV), snap_val=torch.zeros(max(S, 1), G, k, device=DEV))
    tp = Tape(DEV)
    tp.pc_orthonormalise(jd=d["jd"], mask=d["mask"], unit=d["unit"], previous=d["previous"], probe=d["probe"], state=state,
                         stats=d["stats"], tab=d["tab"], G=G, k=k, N=N, iters=iters, const=const,
                         snap_vec=d["snap_vec"] if S else None, snap_val=d["snap_val"] if S else None, S=S, it_imm=it)
    tp.run()
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in d.items()}


def _fp32_product_path(jd, mask4, toe, k):
    """What the per-timestep path computes today, in fp32 on the CPU: (sorted unit [k, N], lengths [k])."""
    len32 = pc_drift._masked_lengths(jd, mask4, k)
    if k > 1:
        unit = pc_drift._orthonormal_rows((jd / len32.reshape(k, 1, 1, 1)) * mask4)
        unit = unit[(len32 * toe).reshape(k).sort(descending=True, stable=True)[1], ...]
    else:
        unit = (jd / len32) * mask4
    return unit.reshape(k, -1), len32.reshape(k)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_orthonormalise_against_fp64(shape):
    """Per column |q - q64| <= 3 |q32 - q64| + 1e-6 and per length |len - len64| / len64 <= 3 e32 + 2^-22, q32 / e32 being
    pc_drift._orthonormal_rows / _masked_lengths in fp32 on the CPU.  Signs are part of the comparison everywhere except in
    the ill-conditioned set (columns = one direction + 1e-3 noise) where the fp64 pivots are within 100 fp32 column errors
    of zero."""
    C, H, W = shape
    N = C * H * W
    gen = torch.Generator().manual_seed(N + 1)
    const = 1e-2
    worst = dict(q=0.0, length=0.0)
    for mname, mask3 in _masks(C, H, W).items():
        mask, mask4 = mask3.reshape(N), mask3.reshape(1, C, H, W)
        for G in GS:
            for k in KS:
                for ill in (False, True):
                    jd = torch.randn(G, k, N, generator=gen)
                    if ill:
                        jd = torch.randn(G, 1, N, generator=gen) + 1e-3 * jd
                    jd = jd * torch.rand(G, k, 1, generator=gen).add(0.5)              # distinct lengths
                    tab = _tab(G, gen)
                    prev = torch.randn(G, k, N, generator=gen)
                    got = _orthonormalise(jd, mask, prev, tab, const, it=0)
                    want = ref.pc_orthonormalise(jd.numpy(), mask.numpy(), prev.numpy(), tab.numpy(), const, 0)
                    tag = (shape, mname, G, k, ill)
                    assert torch.equal(got["previous"], got["unit"]), tag
                    assert torch.equal(got["probe"], got["unit"] * torch.tensor(const, dtype=torch.float32)), tag
                    assert torch.isfinite(got["unit"]).all(), tag
                    for g in range(G):
                        q32, len32 = _fp32_product_path(jd[g].reshape(k, C, H, W), mask4, tab[g, 3], k)
                        q64, len64 = want["unit"][g], want["lengths"][g]
                        q = got["unit"][g].double().numpy()
                        e32 = np.abs(len32.double().numpy() - len64) / len64
                        e_len = np.abs(got["stats"][0, 0, g].double().numpy() - len64) / len64
                        assert (e_len <= 3 * e32 + 2.0 ** -22).all(), (tag, g, e_len, e32)
                        err32 = np.linalg.norm(q32.double().numpy() - q64, axis=1)
                        err = np.linalg.norm(q - q64, axis=1)
                        if ill and k > 1 and want["margin"][g] < 100 * err32.max():
                            err32 = np.minimum(err32, np.linalg.norm(q32.double().numpy() + q64, axis=1))
                            err = np.minimum(err, np.linalg.norm(q + q64, axis=1))
                        assert (err <= 3 * err32 + 1e-6).all(), (tag, g, err, err32, want["margin"][g])
                        worst["q"] = max(worst["q"], float((err / (3 * err32 + 1e-6)).max()))
                        worst["length"] = max(worst["length"], float((e_len / (3 * e32 + 2.0 ** -22)).max()))
    print("pc_orthonormalise vs fp64, worst fraction of the bound:", shape, worst)


def test_orthonormalise_sort_statistics_and_snapshots():
    """41 iterations from a device counter with a stub in place of the U-Net (a fresh jd per iteration, directions 0 and 1
    of equal length): the stable sort, in_norm, in_corr, the snapshot slots of iterations 20, 30 and 40, and no write at all
    from an iteration beyond `iters`."""
    C, H, W = 8, 5, 3
    G, k, N, iters, S, const = 3, 4, 8 * 5 * 3, 41, 3, 1e-3
    gen = torch.Generator().manual_seed(5)
    mask = _masks(C, H, W)["tail"].reshape(N)
    tab = _tab(G, gen)
    d = dict(jd=torch.zeros(G, k, N, device=DEV), mask=mask.to(DEV), unit=torch.zeros(G, k, N, device=DEV),
             previous=torch.randn(G, k, N, generator=gen).to(DEV), probe=torch.zeros(G, k, N, device=DEV),
             stats=torch.zeros(2, iters, G, k, device=DEV), tab=tab.to(DEV), snap_vec=torch.zeros(S, G, k, N, device=DEV),
             snap_val=torch.zeros(S, G, k, device=DEV), state=torch.zeros(4, dtype=torch.int32, device=DEV))
    tp = Tape(DEV)
    tp.pc_orthonormalise(jd=d["jd"], mask=d["mask"], unit=d["unit"], previous=d["previous"], probe=d["probe"],
                         state=d["state"], stats=d["stats"], tab=d["tab"], G=G, k=k, N=N, iters=iters, const=const,
                         snap_vec=d["snap_vec"], snap_val=d["snap_val"], S=S)
    tp.advance(d["state"])
    toe = tab[:, 3]
    for it in range(iters + 1):
        jd = torch.randn(G, k, N, generator=gen) * torch.tensor([1.0, 1.0, 3.0, 0.5]).reshape(1, k, 1)
        jd[:, 1] = jd[:, 0] * torch.sign(torch.randn(N, generator=gen))       # the same squares in the same order: a tie
        prev = d["previous"].cpu().clone()
        before = {n: d[n].clone() for n in ("stats", "snap_vec", "snap_val")}
        d["jd"].copy_(jd)
        tp.run()
        torch.cuda.synchronize()
        unit = d["unit"].cpu().clone()
        if it == iters:                                  # beyond the statistics' rows: nothing is written there
            assert all(torch.equal(before[n], d[n]) for n in before)
            break
        want = ref.pc_orthonormalise(jd.numpy(), mask.numpy(), prev.numpy(), tab.numpy(), const, it)
        len_dev = d["stats"][0, it].cpu()
        assert (len_dev[:, 0] == len_dev[:, 1]).all()
        np.testing.assert_allclose(len_dev.numpy(), want["lengths"], rtol=2.0 ** -22)
        assert np.abs(unit.numpy() - want["unit"]).max() < 1e-5, it      # sorted as [2, 0, 1, 3]: the tie keeps its order
        for g in range(G):
            first = ref.orthonormal_rows((jd[g].double() / len_dev[g].double()[:, None] * mask).numpy())[0]
            assert np.abs(unit[g].numpy() - first[[2, 0, 1, 3]]).max() < 1e-5, (it, g)
        if it > 0:
            corr = (prev.double() * unit.double()).sum(-1)
            np.testing.assert_allclose(d["stats"][1, it - 1].cpu().numpy(), corr.numpy(), atol=1e-6)
        if it in (20, 30, 40):
            assert torch.equal(d["snap_vec"][it // 10 - 2].cpu(), unit), it
            assert torch.equal(d["snap_val"][it // 10 - 2].cpu(), len_dev * toe.reshape(G, 1)), it
        else:
            assert torch.equal(before["snap_vec"], d["snap_vec"]) and torch.equal(before["snap_val"], d["snap_val"]), it
    assert int(d["state"][0]) == iters + 1
    assert (d["stats"][1, iters - 1] == 0).all() and (d["stats"][0] > 0).all()


# ------------------------------------------------------------------------------------------------ end to end
T, N_EV, CONST, CFG = 50, 4, 1e-2, 3.0


@pytest.fixture(scope="module")
def setup():
    """tiny/audioldm2, T = 50, k 4, const 1e-2, CPU-drawn start vectors, the mask of test_gpu_pc, three consecutive window
    timesteps.  Computed once and left unchanged.

    x_t, the step noise and the start vectors are the draws of test_gpu_pc.test_power_iteration_and_drift_match_oracle (same
    generator, same order), used at its timestep (index 30) and the two that follow: the oracle thresholds applied below were
    set on that input, and an input decides whether the EXISTING path meets them.  They are per INDEX, and get_eigenvectors
    reports the eigenvalues in the order the PREVIOUS iteration's sort left them, so two estimates closer to each other than
    the HIP and CPU forwards are can change places between two stacks.  The figures that led here are consistent with that
    (two neighbouring entries off by the same amount, on both HIP paths alike): with fresh draws per slot (seed 3: four x_t, the noise, four start tensors; timesteps 29-31) one
    slot had its third and fourth eigenvalue 5.8 % / 5.0 % off the oracle on the per-timestep path and 5.3 % / 4.9 % on the
    window path after 4 iterations (all vectors |cos| > 0.9992, 4e-5 after 1 iteration), the other two slots at most 0.7 %."""
    from oracle import loops as oloops, pc as opc, unet as ounet
    from oracle.scheduler import OracleDDIMScheduler
    m = models.load_model("tiny/audioldm2", DEV, T, seed=0)
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
    ts = m.model.scheduler.timesteps[30:33]
    xt = torch.randn(1, 8, 32, 16, generator=g) * 0.8
    latent = torch.randn(1, 8, 32, 16, generator=g)
    init = torch.randn(N_EV, 8, 32, 16, generator=g)
    xts, inits = [xt] * 3, [init] * 3
    mask = torch.ones_like(xt)
    mask[..., 12:] = 0
    emb = lambda p: PromptEmbeddings(embedding_hidden_states=m.encode_text(p)[0], embedding_class_lables=m.encode_text(p)[1],   # noqa: E731
                                     boolean_prompt_mask=m.encode_text(p)[2])
    c_unc, c_txt = m.encode_text([""]), m.encode_text(["a dog barking"])
    x0s = [opc.forward_directional(ow, x, t, latent, c_unc, c_txt, CFG, eta=1.0)[1] * mask for x, t in zip(xts, ts)]
    return dict(m=m, ow=ow, opc=opc, ts=ts, xts=xts, latent=latent, inits=inits, mask=mask, e_unc=emb([""]),
                e_txt=emb(["a dog barking"]), c_unc=c_unc, c_txt=c_txt, x0s=x0s)


def _window(s, n, iters, n_ev=N_EV, mode=pc_drift.PCStreamChoice.BOTH, inits=None):
    inits = [v[:n_ev] for v in s["inits"][:n]] if inits is None else inits
    return pc_drift.get_eigenvectors_window(s["m"], [x.to(DEV) for x in s["xts"][:n]], s["e_txt"], s["e_unc"], s["mask"].to(DEV),
                                            s["ts"][:n], [x.to(DEV) for x in s["x0s"][:n]], mode, CONST, CFG, iters, 1.0, n_ev,
                                            init_eigvecs=inits)


def _single(s, j, iters, n_ev=N_EV, mode=pc_drift.PCStreamChoice.BOTH):
    return pc_drift.get_eigenvectors(s["m"], s["xts"][j].to(DEV), s["e_txt"], s["e_unc"], s["latent"].to(DEV),
                                     s["mask"].to(DEV), s["ts"][j], s["x0s"][j].to(DEV), pc_mode=mode, const=CONST,
                                     cfg_tar=CFG, iters=iters, eta=1.0, n_ev=n_ev, init_eigvecs=s["inits"][j][:n_ev])


def _same_layout(a, b):
    """Two get_eigenvectors tuples with the same shapes, dtypes and devices, entry by entry."""
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert list(x) == list(y)
            x, y = list(x.values()), list(y.values())
        if isinstance(x, list):
            assert len(x) == len(y)
        for u, v in zip(*((x, y) if isinstance(x, list) else ([x], [y]))):
            assert u.shape == v.shape and u.dtype == v.dtype and u.device == v.device, (u.shape, v.shape, u.device, v.device)


def _cos(a, b):
    k = a.shape[0]
    return (a.reshape(k, -1).cpu().double() * b.reshape(k, -1).cpu().double()).sum(1)


@pytest.mark.parametrize("iters", [1, 4])
def test_window_matches_the_oracle_no_worse_than_the_per_timestep_path(setup, iters):
    """Three timesteps x 4 directions in one loop against oracle.pc.get_eigenvectors per timestep, under the thresholds of
    test_power_iteration_and_drift_match_oracle; and for the eigenvalue error and 1 - min |cos| the window path may be at
    most 2 x the per-timestep HIP path + 1e-5 (two fp32 forwards of one network that differ in tile choice)."""
    s = setup
    got = _window(s, 3, iters)
    rep = lambda c: tuple(v.repeat(N_EV, *[1] * (v.dim() - 1)) for v in c)                        # noqa: E731
    rows = []
    for j in range(3):
        ev_o, val_o, _, _ = s["opc"].get_eigenvectors(s["ow"], s["xts"][j], rep(s["c_txt"]), rep(s["c_unc"]), s["latent"],
                                                      s["mask"], s["ts"][j], s["x0s"][j], s["inits"][j], const=CONST, cfg_tar=CFG,
                                                      iters=iters, eta=1.0, n_ev=N_EV)
        val_o = torch.as_tensor(val_o).reshape(-1)
        one = _single(s, j, iters)
        _same_layout(got[j], one)
        for name, (ev, val, corr, nrm, _, _) in (("window", got[j]), ("single", one)):
            assert ev.shape == (N_EV, 8, 32, 16) and len(corr) == iters - 1 and len(nrm) == iters
            gram = ev.reshape(N_EV, -1) @ ev.reshape(N_EV, -1).T
            rows.append(dict(path=name, slot=j, gram=float((gram.cpu() - torch.eye(N_EV)).abs().max()),
                             eigval_rel=((val.cpu().reshape(-1) - val_o).abs() / val_o.abs()).tolist(),
                             cos=_cos(ev, ev_o).abs().tolist()))
        rows.append(dict(path="between", slot=j, cos=_cos(got[j][0], one[0]).tolist()))
    worst = {name: dict(eigval=max(max(r["eigval_rel"]) for r in rows if r["path"] == name),
                        one_minus_cos=max(1 - min(r["cos"]) for r in rows if r["path"] == name)) for name in ("window", "single")}
    print(f"window vs per-timestep against the oracle, iters {iters}:", worst)
    for r in rows:
        print("   ", r)
    for r in rows:
        if r["path"] == "between":
            assert min(r["cos"]) > 0.99, r                 # the two HIP paths, sign included
            continue
        assert r["gram"] < 1e-4, r
        assert max(r["eigval_rel"]) <= 5e-2, r
        assert min(r["cos"]) > 0.99, r
    for key in ("eigval", "one_minus_cos"):
        assert worst["window"][key] <= 2 * worst["single"][key] + 1e-5, (key, worst)


@pytest.mark.parametrize("n_ev, mode", [(1, pc_drift.PCStreamChoice.BOTH), (4, pc_drift.PCStreamChoice.TEXT)],
                         ids=["n_ev1", "text"])
def test_window_one_direction_and_text_mode(setup, n_ev, mode):
    s = setup
    got = _window(s, 2, 3, n_ev=n_ev, mode=mode)
    for j in range(2):
        one = _single(s, j, 3, n_ev=n_ev, mode=mode)
        _same_layout(got[j], one)
        if n_ev == 1:
            assert got[j][1].dim() == 0 and got[j][3][0].dim() == 0 and got[j][2][0].shape == (1,)
        assert _cos(got[j][0], one[0]).min() > 0.99
        torch.testing.assert_close(got[j][1], one[1], rtol=5e-2, atol=1e-6)
        for a, b in zip(got[j][3], one[3]):
            torch.testing.assert_close(a, b, rtol=5e-2, atol=1e-7)
    if mode is pc_drift.PCStreamChoice.TEXT:               # another Jacobian than with both streams displaced
        both = _window(s, 2, 3, n_ev=n_ev)
        assert not torch.equal(both[0][3][0], got[0][3][0])


def test_window_is_bit_repeatable_and_snapshots_late_iterates(setup):
    s = setup
    a = _window(s, 3, 21, n_ev=2)
    b = _window(s, 3, 21, n_ev=2)
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
        assert all(torch.equal(u, v) for u, v in zip(x[2] + x[3], y[2] + y[3]))
        assert list(x[4]) == list(x[5]) == [20] and torch.equal(x[4][20], y[4][20]) and torch.equal(x[5][20], y[5][20])
        # iteration 20 is the last of 21: its snapshot is the returned iterate
        assert torch.equal(x[5][20], x[1]) and (x[4][20] - x[0]).abs().max() < 1e-6
    # a slot's result does not depend on the size of its group: the same timesteps in a group of two and of three
    c, d = _window(s, 2, 2, n_ev=2), _window(s, 3, 2, n_ev=2)
    for j in range(2):
        assert _cos(c[j][0], d[j][0]).min() > 0.99
        torch.testing.assert_close(c[j][1], d[j][1], rtol=5e-2, atol=1e-6)


def _extract_args(Tn, start, end, **kw):
    from audioeditingcode_amd import main_pc_extract_inv as pext
    a = pext.finish_args(Namespace(seed=1, cfg_tar=3, model_id="tiny/audioldm2", init_aud=None, num_diffusion_steps=Tn,
                                   source_prompt=["rain"], target_neg_prompt=[""], corr_to_swap=0.8, drift_start=start,
                                   drift_end=end, results_path="unused", const=0.3, n_evs=2, patch=None, iters=2, dry=False))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_extract_pcs_in_groups_with_a_tail(monkeypatch):
    """A 4-step window in groups of 3 (3 + 1) against one timestep at a time: the same checkpoint structure, the same PCs."""
    from audioeditingcode_amd import main_pc_extract_inv as pext
    Tn = 8
    m = models.load_model("tiny/audioldm2", DEV, Tn, seed=0)
    w0 = torch.randn(1, 8, 32, 16, generator=torch.Generator().manual_seed(5)) * 0.7
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: torch.randn(x.shape, dtype=x.dtype).to(x.device))
    cks, cbs = [], []
    for group in (1, 3):
        torch.manual_seed(1)
        cb = []
        cks.append(pext.extract_pcs(m, w0.to(DEV), _extract_args(Tn, 6, 2, timestep_group=group),
                                    checkpoint_cb=lambda st: cb.append(len(st["eigdata"]))))
        cbs.append(cb)
    one, grp = cks
    assert cbs[1] == [3, 4] and list(one["eigdata"]) == list(grp["eigdata"]) and len(grp["eigdata"]) == 4
    assert len(grp["corrs"]) == 3 and len(grp["in_corrs"]) == len(grp["in_norms"]) == 4
    for a, b in zip(one["xts"], grp["xts"]):
        assert torch.equal(a, b)                                                  # the trunk replay is the same code
    for t in one["eigdata"]:
        ea, eb = one["eigdata"][t], grp["eigdata"][t]
        assert ea.keys() == eb.keys() and ea["it"] == eb["it"] and ea["ts"] == eb["ts"]
        assert ea["eigvec"].shape == eb["eigvec"].shape and ea["eigval"].shape == eb["eigval"].shape
        assert _cos(ea["eigvec"], eb["eigvec"]).min() > 0.99, t
        torch.testing.assert_close(ea["eigval"], eb["eigval"], rtol=5e-2, atol=1e-6)
    for a, b in zip(one["corrs"], grp["corrs"]):
        assert (a.cpu() - b.cpu()).abs().max() < 2e-2


def test_extract_and_apply_in_groups_is_as_close_to_the_cpu_stack(monkeypatch):
    """extract_pcs with timestep_group 3 and 1, then apply_pcs, against the CPU tape-interpreter stack's drifted latents (the
    committed run of test_pc_clis_extract_pt_apply_on_the_gpu, same seeds): the grouped extraction may be at most twice as
    far from it as the per-timestep one."""
    from audioeditingcode_amd import main_pc_apply_drift as papply, main_pc_extract_inv as pext
    from conftest import ORACLE_RUNS
    Tn = 6
    w0 = torch.randn(1, 8, 32, 16, generator=torch.Generator().manual_seed(5)) * 0.7
    blob = torch.load(os.path.join(ORACLE_RUNS, "pc_cli_cpu_stack_T6.pt"), map_location="cpu", weights_only=False)
    assert torch.equal(blob["probe"], w0)
    out_c = blob["out"]["out"]
    ap = Namespace(drift_start=5, drift_end=3, amount=1.5, use_specific_ts_pc=None, fix_alpha=None, fade_length=0.0,
                   evs=[1, 2], combine_evs=False, evals_pt=None, rand_v=False, shift_x0_for_np=True, sub_iters=None)
    keys = ("eigdata", "args", "corrs", "in_corrs", "latents", "in_norms", "xts")
    m = models.load_model("tiny/audioldm2", DEV, Tn, seed=0)
    monkeypatch.setattr(torch, "randn_like", lambda x, **kw: torch.randn(x.shape, dtype=x.dtype).to(x.device))
    dist = {}
    for group in (1, 3):
        torch.manual_seed(1)
        ck = pext.extract_pcs(m, w0.to(DEV), _extract_args(Tn, 5, 3, timestep_group=group))
        out = papply.apply_pcs(m, {k: ck[k] for k in keys}, ap, torch.device(DEV)).cpu()
        dist[group] = ((out - out_c).norm() / out_c.norm()).item()
    print("drifted latents against the CPU stack, relative L2 by timestep_group:", dist)
    assert dist[1] < 8e-3                                                          # the existing test's bound
    assert dist[3] <= 2 * dist[1], dist
