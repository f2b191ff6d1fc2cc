"""CPU: tests/body_grad_ref.py (the torch restatement of the two body-model forwards, differentiated by autograd) reproduces
the gradients the real SMPL_Layer / ManoLayer produced (tests/golden/body_grad_*.npz), and the fixtures cover what the
kernels can trip on."""
import os

import numpy as np
import pytest
import torch

import body_cases
import body_grad_cases
import body_grad_ref
import body_ref


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("flavour,name", body_cases.case_ids())
def test_body_grad_ref_reproduces_fixture(flavour, name):
    c = body_grad_cases.case(flavour, name)
    got = body_grad_ref.grads(c["model"], c["pose"], c["betas"], c["trans"], c["center_idx"], c["extra_reg"], coeffs=c["coeffs"])
    for n, g, w, given in zip(body_grad_cases.NAMES, got, c["grads"], (c["pose"], c["betas"], c["trans"])):
        assert (g is None) == (w is None) == (given is None), n
        if w is not None:
            assert g.shape == w.shape == given.shape and np.isfinite(w).all() and _rel(g, w) <= 1e-12, (n, _rel(g, w))


@pytest.mark.parametrize("flavour,name", [("smpl", "rand_b5"), ("mano", "b5")])
def test_torch_forward_equals_numpy_forward(flavour, name):
    c = body_cases.case(flavour, name)
    a = body_grad_ref.forward(c["model"], c["pose"], c["betas"], c["trans"], c["center_idx"], c["extra_reg"])
    b = body_ref.forward(c["model"], c["pose"], c["betas"], c["trans"], c["center_idx"], c["extra_reg"])
    assert len(a) == len(b) and all(_rel(x.numpy(), y) <= 1e-13 for x, y in zip(a, b))


def test_fixtures_cover_the_issue_cases():
    ids = body_cases.case_ids()
    cs = [body_grad_cases.case(f, n) for f, n in ids]
    assert {c["pose"].shape[0] for c in cs} == {1, 5, 37}
    assert {c["model"]["kind"] for c in cs} == {"smpl", "chain", "star", "mano"}
    for flavour in ("smpl", "mano"):
        fc = [c for (f, _), c in zip(ids, cs) if f == flavour]
        assert {c["grads"][2] is None for c in fc} == {True, False} and {c["center_idx"] for c in fc} == {None, 0}
        assert any(c["grads"][1] is None for c in fc) and any(len(c["coeffs"]) == 3 for c in fc)
        zero = [(c, int(np.flatnonzero((c["pose"] == 0).all(axis=1))[0])) for c in fc if (c["pose"] == 0).all(axis=1).any()]
        assert zero and all(np.isfinite(c["grads"][0][i]).all() and np.abs(c["grads"][0][i]).max() > 0 for c, i in zero)
        assert any(np.linalg.norm(c["pose"].reshape(-1, 3), axis=1).max() > np.pi for c in fc)
        assert any(c["betas"] is not None and np.abs(c["betas"]).max() > 3 for c in fc)
        # the reference's own fp32 autograd is fp32-class on every row, the zero pose and the angles beyond pi included
        worst = body_grad_cases.file_gerr32(flavour)
        assert set(worst) == {"pose", "betas", "trans"} and all(0 < e < 5e-6 for e in worst.values()), worst
    assert all(os.path.getsize(os.path.join(body_cases.GOLDEN, f)) < 1 << 20 for f in body_grad_cases.FILES.values())


def test_fp32_mode_runs_in_fp32():
    c = body_grad_cases.case("smpl", "rand_b5")
    out = body_grad_ref.forward(c["model"], c["pose"], c["betas"], c["trans"], dtype=torch.float32)
    assert all(o.dtype == torch.float32 for o in out)
    g4 = body_grad_ref.grads(c["model"], c["pose"], c["betas"], c["trans"], coeffs=c["coeffs"][:2], dtype=torch.float32)
    g8 = body_grad_ref.grads(c["model"], c["pose"], c["betas"], c["trans"], coeffs=c["coeffs"][:2])
    for a, b in zip(g4, g8):
        assert 0 < body_grad_ref.row_err(a, b) < 5e-6
