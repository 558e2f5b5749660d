"""Codelength the device's Infomap search reaches over the codelength the sequential numpy model reaches
(tests/infomap_hostmodel.py), on the test fixtures and a few noisier blob graphs small enough for the model: one line per
graph.  Both searches are local searches of the same objective from the same start; neither bounds the other, so the ratio is
reported and nothing is asserted about it.  Both codelengths are the model's L of the respective partition on the device's
flow.  usage: python tools/infomap_codelength_ratio.py > profiles/infomap_codelength.txt"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "reid-gan_amd"))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from rg_hip import ops  # noqa: E402
from tests import infomap_hostmodel as M  # noqa: E402

dev = torch.device("cuda", 0)
GRAPHS = [("ring %dx%d" % cs, M.ring_of_cliques(*cs), 0.5) for cs in M.RINGS]
GRAPHS.append(("ring 3x5 + dangling, source-only and isolated node", M.ring_with_extras(3, 5), 0.5))
for args, min_sim in (((10, 8, 32, 0.08, 10), 0.5), ((20, 8, 64, 0.1, 12), 0.5), ((12, 6, 16, 0.15, 8), 0.6), ((12, 6, 16, 0.3, 8), 0.6),
                      ((15, 10, 16, 0.35, 10), 0.4), ((30, 6, 8, 0.25, 8), 0.3)):
    GRAPHS.append(("blobs %d x %d in %d-d sigma %.2f k %d min_sim %.1f" % (args + (min_sim,)), M.blob_table(*args), min_sim))
GRAPHS.append(("blobs 5 x 8 in 4-d sigma 0.70 k 10 min_sim 0.05 seed 4 (one sweep rolled back)", M.blob_table(5, 8, 4, 0.7, 10, seed=4), 0.05))

print("graph | nodes links | L device | L sequential model | ratio | L planted | modules device / model | sweeps levels rollbacks converged")
for name, (nbrs, dists, planted), min_sim in GRAPHS:
    N = nbrs.shape[0]
    tn, td = torch.from_numpy(nbrs).to(dev), torch.from_numpy(dists).to(dev)
    labels, info = ops.infomap(tn, td, min_sim, 0)
    g = ops.infomap_flow(ops.infomap_links(tn, td, min_sim))
    src, dst = g["src"].cpu().numpy().astype(np.int64), g["dst"].cpu().numpy().astype(np.int64)
    q, node_flow = g["q"].cpu().numpy(), g["flow"].cpu().numpy()
    got = info["modules"].cpu().numpy()
    seq = M.search(N, src, dst, q, node_flow)
    Ld, Ls = M.codelength(src, dst, q, node_flow, got), M.codelength(src, dst, q, node_flow, seq)
    print("%s | %d %d | %.6f | %.6f | %.6f | %.6f | %d / %d | %d %d %d %s" % (
        name, N, len(src), Ld, Ls, Ld / Ls, M.codelength(src, dst, q, node_flow, planted), len(set(got.tolist())),
        len(set(seq.tolist())), info["sweeps"], info["levels"], info["rollbacks"], info["converged"]))
