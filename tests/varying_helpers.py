"""Shared by tests/test_padded_batch_cpu.py and tests/test_varying_topology_gpu.py: small batches of changing topology and
the padded forms of the committed model fixtures."""
import numpy as np
import torch

# per-simplex feature tensors of the four task models' batches (they get zero filler rows)
SIMPLEX_FEATURES = {"md17": ("loc", "vel", "charges"), "motion": ("pos", "vel"), "nba": ("pos", "vel"), "hulls": ("input",)}
# rows per dimension | adjacencies of rips_batch(seed) and of test_model_harness._hull_batch(seed)
RIPS_COUNTS = {1: ((24, 25, 11), 377), 2: ((24, 20, 8), 316), 3: ((24, 19, 8), 311), 4: ((24, 17, 3), 241)}
HULL_COUNTS = {9: ((32, 110, 200), 3174), 10: ((32, 109, 196), 3121)}
SPARE = ((3, 2), 7)      # spare 1-simplices, 2-simplices | adjacencies of the padded model fixtures


def rips_batch(seed, n_graphs=4, points=6, dis=1.6, max_dim=2, md17=False):
    """Vietoris-Rips complexes of `points` standard normal points in R^3 each; md17: with the feature tensors of the md17
    model (10 frames: loc, vel, charges per simplex row - vertex rows filled - and the per-vertex target y)."""
    from csmpn.data import complexes as cx
    rng = np.random.default_rng(seed)
    F, graphs = 10, []
    for _ in range(n_graphs):
        base = rng.standard_normal((points, 3))
        c = cx.rips_complex(base, dis=dis, max_dim=max_dim)
        if md17:
            S, V = c.n_simplices, points
            loc, vel, ch = torch.zeros(S, F, 3), torch.zeros(S, F, 3), torch.zeros(S, F, 1)
            loc[:V] = torch.from_numpy(base.astype(np.float32))[:, None, :] + 0.05 * torch.from_numpy(rng.standard_normal((V, F, 3)).astype(np.float32))
            vel[:V] = 0.1 * torch.from_numpy(rng.standard_normal((V, F, 3)).astype(np.float32))
            ch[:V] = torch.from_numpy(rng.integers(1, 9, size=(V, 1, 1)).astype(np.float32)).expand(V, F, 1)
            c.features.update(loc=loc, vel=vel, charges=ch)
        graphs.append(c)
    b = cx.collate(graphs)
    if md17:
        b.y = torch.cat([g.features["loc"][:points] + 0.1 * torch.from_numpy(rng.standard_normal((points, F, 3)).astype(np.float32))
                         for g in graphs], dim=0)
        b._names.append("y")
    return b


def counts_of(batch, max_dim=2):
    return tuple(torch.bincount(batch.node_types, minlength=max_dim + 1).tolist()), int(batch.edge_index.shape[1])


def spare_capacity(batch, max_dim=2):
    """The batch's own counts + SPARE."""
    from csmpn.data.complexes import BatchCapacity
    rows, edges = counts_of(batch, max_dim)
    return BatchCapacity((rows[0],) + tuple(r + s for r, s in zip(rows[1:], SPARE[0])), edges + SPARE[1])


def padded_fixture(kind, batch):
    from csmpn.data.complexes import pad_batch
    return pad_batch(batch, spare_capacity(batch), SIMPLEX_FEATURES[kind])
