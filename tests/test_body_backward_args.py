"""CPU: p2m_body_backward checks its arguments before any launch (no GPU needed), p2m_body_backward_workspace sizes the
per-block partials, and the host side of body.BodyLayer builds the tables the backward reads."""
import ctypes

import numpy as np
import pytest
import torch

import body_cases
from pose2mesh_release_amd import _lib, body, synth


def test_backward_workspace(hip_libs):
    ws = _lib.hip().p2m_body_backward_workspace
    # per vertex block and sample: 12 (J + 1) doubles of g_A, then K (rounded up to 4) floats of g_coef
    assert ws(3, 6890, 24, 10) == 108 * 3 * (24 * 25 + 220) * 4
    assert ws(1, 1, 1, 1) == (24 * 2 + 4) * 4 and ws(1, 64, 2, 0) == (24 * 3 + 12) * 4 and ws(1, 65, 2, 0) == 2 * (24 * 3 + 12) * 4
    assert ws(0, 1, 1, 1) < 0 and ws(1, 0, 1, 1) < 0 and ws(1, 1, 65, 10) < 0 and ws(1, 1, 1, 0) < 0 and ws(1, 1, 64, 74) < 0


def test_c_entry_rejects_bad_arguments(hip_libs):
    lib = _lib.hip()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok = dict(pose=base, pose_mean=None, betas=base, per=1, has_trans=1, center=-1, scale=1.0, B=1, V=1, J=2, nb=1,
              tmpl=base, dirs=base, dirs_t=base, wt=base, jt=base, js=base, parents=base, jslot=base, NJ=2, tv=None, ts=None,
              nt=0, xp=None, xi=None, xv=None, nx=0, fws=base, fwsb=1 << 20, gv=base, gj=None, gx=None, ws=base, wsb=1 << 20,
              gpose=base, gbetas=base, gtrans=base, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.p2m_body_backward(*[a[k] for k in ok])
    for kw, word in ((dict(pose=None), "null"), (dict(fws=None), "null"), (dict(ws=None), "null"), (dict(B=0), ">= 1"),
                     (dict(V=0), ">= 1"), (dict(J=65), "64"), (dict(nb=640), "640"), (dict(center=2), "center_joint"),
                     (dict(nt=1), "tips"), (dict(nx=1, gx=base), "extra"), (dict(gx=base), "g_extra"),
                     (dict(gpose=None, gbetas=None, gtrans=None), "no gradient output"), (dict(gv=None), "no upstream"),
                     (dict(has_trans=0), "g_trans"), (dict(per=0), "g_betas"), (dict(dirs_t=None), "dirs_t"),
                     (dict(gv=base + 2), "misaligned"), (dict(gpose=base + 2), "misaligned"), (dict(ws=base + 4), "misaligned"),
                     (dict(fws=base + 8), "misaligned"), (dict(fwsb=8), "forward workspace"), (dict(wsb=8), "p2m_body_backward_workspace")):
        assert call(**kw) != 0, kw
        assert word in lib.p2m_last_error_string().decode(), (kw, lib.p2m_last_error_string())


def test_gradient_tables():
    """The vertex-major direction table and the regressor by column, as BodyLayer's first call uploads them."""
    m = body_cases.model("smpl", 65)
    reg = synth.synthetic_regressor(5, 65, seed=4)
    model = body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"],
                           extra_regressor=reg)
    g = {k: v.numpy() for k, v in model._grad_tables(torch.device("cpu")).items()}
    assert g["dirs_t"].shape == (195, 220) and g["dirs_t"].dtype == np.float32
    assert np.array_equal(g["dirs_t"][:, :217], model._host["dirs"].T) and not g["dirs_t"][:, 217:].any()
    assert g["dirs_t"][7 * 3 + 2, 3] == m["shapedirs"][7, 2, 3] and g["dirs_t"][64 * 3 + 1, 110] == m["posedirs"][64, 1, 100]
    dense = np.zeros((5, 65), np.float32)
    for v in range(65):
        e = slice(g["xc_ptr"][v], g["xc_ptr"][v + 1])
        assert (np.diff(g["xc_idx"][e]) > 0).all()                            # joints ascending within a vertex
        dense[g["xc_idx"][e], v] = g["xc_val"][e]
    assert np.array_equal(dense, reg) and g["xc_ptr"].shape == (66,)
    plain = body.BodyModel(m["v_template"], m["shapedirs"], m["posedirs"], m["J_regressor"], m["weights"], m["parents"])
    assert set(plain._grad_tables(torch.device("cpu"))) == {"dirs_t"}
    with pytest.raises(TypeError):
        body.BodyLayer(m)
    assert not list(body.BodyLayer(plain).parameters())
