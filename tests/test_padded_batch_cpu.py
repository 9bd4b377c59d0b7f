"""Fixed-capacity batches (csmpn.data.complexes: BatchCapacity, capacity_of, pad_batch), no GPU needed: the layout of a
padded batch, the host-side validation, and the four task models on the padded forms of their committed fixture batches
(the oracle standing in for the HIP layers, as in tests/test_model_harness.py) - filler simplices and filler adjacencies
must not move a single reference result."""
import os

import numpy as np
import pytest
import torch

import test_model_harness as H
import varying_helpers as V
from test_model_harness import oracle_layers  # noqa: F401  (fixture)


def _batches(pkg, family):
    if family == "rips":
        return {s: V.rips_batch(s) for s in V.RIPS_COUNTS}, V.RIPS_COUNTS, ()
    return {s: H._hull_batch(pkg, s) for s in V.HULL_COUNTS}, V.HULL_COUNTS, ("input",)


@pytest.mark.parametrize("family", ["rips", "hulls"])
def test_padded_layout(pkg, family):
    from csmpn.data import complexes as cx
    batches, want, feats = _batches(pkg, family)
    for s, b in batches.items():
        assert V.counts_of(b) == want[s], (s, V.counts_of(b))
    cap = cx.capacity_of(list(batches.values()))
    rows = [max(want[s][0][d] for s in want) for d in range(3)]
    assert cap == cx.BatchCapacity((rows[0], rows[1] + 1, rows[2]), max(want[s][1] for s in want))   # one spare 1-simplex
    assert cx.capacity_of(list(batches.values()), slack=0.5).simplices[0] == rows[0]                # vertex rows: never
    for s, b in batches.items():
        p = cx.pad_batch(b, cap, feats)
        S, E, B = int(b.node_types.shape[0]), int(b.edge_index.shape[1]), b.num_graphs
        assert (p.n_real_rows, p.n_real_edges) == (S, E)
        # shapes = the capacity's
        assert p.node_types.shape == (cap.rows,) and p.x_ind.shape == (cap.rows, 3) and p.batch.shape == (cap.rows,)
        assert p.x_ind_batch.shape == (cap.rows,) and p.edge_index.shape == (2, cap.edges) and p.edge_types.shape == (cap.edges, 2)
        assert V.counts_of(p) == (cap.simplices, cap.edges)
        # the real prefix and ptr are unchanged
        for k in ("x_ind", "node_types", "batch", "x_ind_batch") + feats:
            assert torch.equal(getattr(p, k)[:S], getattr(b, k)), k
        assert torch.equal(p.edge_index[:, :E], b.edge_index) and torch.equal(p.edge_types[:E], b.edge_types)
        assert torch.equal(p.ptr, b.ptr) and torch.equal(p.x_ind_ptr, b.x_ind_ptr) and int(p.ptr[-1]) == S
        for k in b._names:
            if k not in ("x_ind", "node_types", "batch", "x_ind_batch", "edge_index", "edge_types") + feats:
                assert torch.equal(getattr(p, k), getattr(b, k)), k
        # fillers: dimension by dimension behind the last graph, local vertex ids 0..d, graph B - 1, zero features
        ft = p.node_types[S:]
        assert torch.equal(ft, torch.sort(ft).values) and int(ft.min()) >= 1
        assert torch.equal(p.x_ind[S:], torch.where(torch.arange(3)[None] <= ft[:, None], torch.arange(3)[None], torch.tensor(0)))
        assert bool((p.batch[S:] == B - 1).all()) and bool((p.x_ind_batch[S:] == B - 1).all())
        for k in feats:
            assert not bool(getattr(p, k)[S:].any())
        # filler adjacencies: self-loops on filler rows, round-robin, typed (d, d); none joins a filler and a real row
        fe = p.edge_index[:, E:]
        assert torch.equal(fe[0], fe[1]) and torch.equal(fe[0], S + torch.arange(cap.edges - E) % (cap.rows - S))
        assert torch.equal(p.edge_types[E:], torch.stack([p.node_types[fe[0]]] * 2, dim=1))
        assert not bool(((p.edge_index[0] >= S) != (p.edge_index[1] >= S)).any())
        # plan() of the padded batch: the capacity's lengths
        plan = p.plan(2)
        assert [int(r.shape[0]) for r in plan["rows"]] == list(cap.simplices)
        assert [tuple(v.shape) for v in plan["verts"]] == [(cap.simplices[0], 1), (2 * cap.simplices[1], 2), (6 * cap.simplices[2], 3)]
        assert torch.equal(plan["vertices_per_graph"], b.plan(2)["vertices_per_graph"])
        # padding a padded batch again: from its real part
        again = cx.pad_batch(p, cap, feats)
        assert all(torch.equal(getattr(again, k), getattr(p, k)) for k in p._names)
        assert cx.capacity_of([p]) == cx.capacity_of([b])


def test_pad_batch_validation(pkg):
    from csmpn.data import complexes as cx
    b = V.rips_batch(1)
    (n0, n1, n2), E = V.counts_of(b)
    cap = cx.BatchCapacity((n0, n1 + 2, n2 + 1), E + 5)
    cx.pad_batch(b, cap)                                                    # fits

    def broken(name, fn):
        c = cx.SimplicialBatch(**{k: getattr(b, k).clone() for k in b._names})
        fn(getattr(c, name))
        return c

    cases = {
        "node_types above max_dim": broken("node_types", lambda t: t.__setitem__(-1, 3)),
        "negative node_types": broken("node_types", lambda t: t.__setitem__(0, -1)),
        "x_ind outside its graph": broken("x_ind", lambda t: t.__setitem__((-1, 0), 6 + 25)),
        "negative x_ind": broken("x_ind", lambda t: t.__setitem__((3, 1), -1)),
        "edge_index past the rows": broken("edge_index", lambda t: t.__setitem__((1, 7), n0 + n1 + n2)),
        "negative edge_index": broken("edge_index", lambda t: t.__setitem__((0, 0), -1)),
        "x_ind_batch past the graphs": broken("x_ind_batch", lambda t: t.__setitem__(-1, 4)),
    }
    for why, c in cases.items():
        with pytest.raises(ValueError):
            cx.pad_batch(c, cap)
            pytest.fail(why)
    for why, bad_cap in {
        "another vertex count": cx.BatchCapacity((n0 + 1, n1 + 2, n2 + 1), E + 5),
        "too many 1-simplices": cx.BatchCapacity((n0, n1 - 1, n2 + 1), E + 5),
        "too many 2-simplices": cx.BatchCapacity((n0, n1 + 2, n2 - 1), E + 5),
        "too many adjacencies": cx.BatchCapacity((n0, n1 + 2, n2 + 1), E - 1),
        "filler adjacencies without a filler row": cx.BatchCapacity((n0, n1, n2), E + 1),
    }.items():
        with pytest.raises(ValueError):
            cx.pad_batch(b, bad_cap)
            pytest.fail(why)
    cx.pad_batch(b, cx.BatchCapacity((n0, n1, n2), E))                      # nothing to fill: fine without a filler row
    with pytest.raises(ValueError):
        cx.pad_batch(b, cap, simplex_features=("no_such_tensor",))
    # the last graph has two vertices: a filler 1-simplex fits, a filler 2-simplex does not
    pts = np.random.default_rng(0).standard_normal((6, 3))
    small = cx.collate([cx.rips_complex(pts, 1.6), cx.rips_complex(pts[:2], 10.0)])
    (m0, m1, m2), Es = V.counts_of(small)
    cx.pad_batch(small, cx.BatchCapacity((m0, m1 + 1, m2), Es + 1))
    with pytest.raises(ValueError):
        cx.pad_batch(small, cx.BatchCapacity((m0, m1 + 1, m2 + 1), Es + 1))


def test_hulls_pooling_ignores_fillers_and_keeps_its_bits(pkg):
    """The composed pooling branch of the hulls model pools over x_ind_ptr ranges: bit-identical to segment_mean on an
    unpadded batch, and blind to the filler rows of a padded one (which carry the last graph's id)."""
    from csmpn.models import simplicial_mpnn as M
    b = H._hull_batch(pkg, 9)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(b.node_types.shape[0], 1, generator=g)
    want = M.segment_mean(x, b.x_ind_batch, b.num_graphs)
    assert torch.equal(M.segment_mean_ptr(x, b.x_ind_batch, b.x_ind_ptr, b.num_graphs), want)
    p = V.padded_fixture("hulls", b)
    xp = torch.cat([x, torch.randn(p.node_types.shape[0] - x.shape[0], 1, generator=g)])
    assert torch.equal(M.segment_mean_ptr(xp, p.x_ind_batch, p.x_ind_ptr, p.num_graphs), want)


@pytest.mark.parametrize("kind", ["md17", "motion", "nba", "hulls"])
def test_padded_fixture_glue_vs_reference_cpu(pkg, oracle_layers, kind):  # noqa: F811
    """The committed fixture batch of every task model, padded with 3 spare 1-simplices, 2 spare 2-simplices and 7 spare
    adjacencies: loss, loss parts and every parameter gradient against the reference's fixture at the tolerances of
    test_*_glue_vs_reference_cpu (hulls forward only, as there)."""
    g = np.load(os.path.join(H.GOLD, f"model_{kind}.npz"))
    model = H.build(pkg, kind, g)
    raw = H.load_batch(pkg, g)
    batch = V.padded_fixture(kind, raw)
    assert batch.node_types.shape[0] == raw.node_types.shape[0] + 5 and batch.edge_index.shape[1] == raw.edge_index.shape[1] + 7
    if kind == "hulls":
        with torch.no_grad():
            loss, parts = model(batch)
        H._check_against_fixture(g, loss, parts, model, grads=False)
    else:
        loss, parts = model(batch)
        loss.backward()
        H._check_against_fixture(g, loss, parts, model)
