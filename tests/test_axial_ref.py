"""Pins tests/axial_ref.py (the float64 reference of test_gpu_axial_attention.py) against the einsum blocks of the project's oracle
(oracle/msa_transformer_oracle.py, tied row attention and column attention) in torch float64, mirrors the product's split rule, and
rehearses every GPU case's noise32 and bound on the CPU: they come from the reference alone."""
import inspect
import math

import numpy as np
import pytest
import torch

import axial_ref as ax
from oracle import msa_transformer_oracle as mo

GRIDS = [(1, 1, 1), (5, 7, 2), (13, 33, 3)]


def test_the_oracle_still_holds_the_blocks_pinned_here():
    src = inspect.getsource(mo.forward_logits)
    for line in ('q = q * ((dh ** -0.5) / math.sqrt(R))', 's = torch.einsum("rihd,rjhd->hij", q, k)', 'ctx = torch.einsum("hij,rjhd->rihd", a, v)',
                 's = torch.einsum("ichd,jchd->hcij", q, k)', 'ctx = torch.einsum("hcij,jchd->ichd", a, v)'):
        assert line in src, line


@pytest.mark.parametrize("R,C,H", GRIDS)
def test_tied_row_attention_matches_the_oracle_block(R, C, H):
    dh, D = 64, 64 * H
    qkv = ax.tied_inputs(R, C, H)
    got, p = ax.tied_row_attention(qkv, R, C, H)
    x = torch.from_numpy(qkv).double().reshape(R, C, 3, H, dh)
    q, k, v = x[:, :, 0] * 8.0, x[:, :, 1], x[:, :, 2]          # the op's q carries the projection's 1/8 = dh^-1/2 already: undo it, ...
    q = q * ((dh ** -0.5) / math.sqrt(R))                        # ... then the oracle's lines
    s = torch.einsum("rihd,rjhd->hij", q, k)
    a = s.softmax(-1)
    ctx = torch.einsum("hij,rjhd->rihd", a, v).reshape(R, C, D)
    assert got.dtype == np.float64 and got.shape == (R * C, D) and p.shape == (H, C, C)
    assert np.abs(p - a.numpy()).max() < 1e-12
    assert np.abs(got - ctx.reshape(R * C, D).numpy()).max() < 1e-11


@pytest.mark.parametrize("R,C,H", GRIDS[1:] + [(2, 1, 1)])
def test_column_attention_matches_the_oracle_block(R, C, H):
    dh, D = 64, 64 * H
    X, W, bias = ax.column_inputs(R, C, H)
    got = ax.column_attention(X, W, bias, R, C, H)
    h = torch.from_numpy(X).double().reshape(C, R, -1).transpose(0, 1)                 # the oracle's order: [R, C, K]
    Wt, bt = torch.from_numpy(W).double(), torch.from_numpy(bias).double()
    proj = [h @ Wt[w * D:(w + 1) * D].T + bt[w * D:(w + 1) * D] for w in range(3)]
    q = (proj[0] * 8.0).view(R, C, H, dh) * (dh ** -0.5)          # the op's q projection carries the 1/8
    k, v = proj[1].view(R, C, H, dh), proj[2].view(R, C, H, dh)
    s = torch.einsum("ichd,jchd->hcij", q, k)
    a = s.softmax(-1)
    ctx = torch.einsum("hcij,jchd->ichd", a, v).reshape(R, C, D)
    assert got.dtype == np.float64
    assert np.abs(got - ctx.transpose(0, 1).reshape(C * R, D).numpy()).max() < 1e-11


def test_fp32_evaluation_stays_fp32():
    qkv = ax.tied_inputs(5, 40, 2)
    lo, plo = ax.tied_row_attention(qkv, 5, 40, 2, np.float32)
    hi, _ = ax.tied_row_attention(qkv, 5, 40, 2)
    assert lo.dtype == np.float32 and plo.dtype == np.float32 and 0 < np.abs(lo - hi).max() < 1e-4
    X, W, bias = ax.column_inputs(40, 3, 2)
    lo, hi = ax.column_attention(X, W, bias, 40, 3, 2, np.float32), ax.column_attention(X, W, bias, 40, 3, 2)
    assert lo.dtype == np.float32 and 0 < np.abs(lo - hi).max() < 1e-4


def test_split_rule_mirror_at_the_values_the_gpu_cases_rely_on():
    assert [ax.tied_splits(*c) for c in ax.TIED_ROW_EDGES] == ax.TIED_ROW_EDGE_SPLITS
    assert ax.tied_splits(18, 300, 12) == 6                       # 3 x 2 tiles x 12 heads = 72: S = 9 would make 648 > 640
    assert ax.tied_splits(400, 287, 12) == 8 and ax.tied_splits(400, 1024, 12) == 2
    assert [ax.tied_kp(C) for C in (1, 63, 64, 65, 1024)] == [64, 64, 64, 128, 1024]


def test_inputs_have_the_properties_the_gpu_file_states():
    R, C, H = 6, 65, 2
    _, p = ax.tied_row_attention(ax.tied_inputs(R, C, H), R, C, H)
    s = np.log(p[:, [c for c in range(C) if c != (2 * C) // 3]][..., :C - 2])           # ordinary rows and keys
    assert 2.0 < (s - s.mean(-1, keepdims=True)).std() < 4.5                            # scores spread by about 3
    assert p[:, (2 * C) // 3].max(-1).min() > 0.5                                       # the spiky query column: one key dominates its row
    assert (p[:, (2 * C) // 3] > 1e-3).sum(-1).max() <= 4                               # ... and all but a few weights vanish


@pytest.mark.parametrize("R,C,H", ax.TIED_CASES + [ax.TIED_FORCED])
def test_rehearse_tied_bounds(R, C, H):
    """noise32 and the bound of every tied case.  The bound's first term is the suite's flat rule; the reference's own fp32 evaluation
    has to stay inside it with room, or the case would test NumPy's summation order instead of the kernel."""
    (ctx, p), (nc, bc), (npr, bp) = ax.tied_reference(ax.tied_inputs(R, C, H), R, C, H)
    print(f"tied rehearsal R={R} C={C} H={H} |ctx|max={np.abs(ctx).max():.2f} noise32={nc:.3e} bound={bc:.3e} | probs noise32={npr:.3e} bound={bp:.3e}")
    assert np.abs(p.sum(-1) - 1).max() < 1e-12
    assert nc < bc and npr < bp
    assert nc < 2e-5 * max(1.0, np.abs(ctx).max()) and npr < 2e-5


@pytest.mark.parametrize("R,C,H", ax.COLUMN_CASES)
def test_rehearse_column_bounds(R, C, H):
    ctx, n, b = ax.column_reference(*ax.column_inputs(R, C, H), R, C, H)
    print(f"column rehearsal R={R} C={C} H={H} |ctx|max={np.abs(ctx).max():.2f} noise32={n:.3e} bound={b:.3e}")
    assert n < b and n < 2e-5 * max(1.0, np.abs(ctx).max())
