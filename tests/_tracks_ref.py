"""NumPy restatement of mvba_build_tracks (include/mvba.h): the connected components of the match graph by min-label
propagation over the edge arrays, the classes of the components, and the output arrays with their codes.  Written from the
header's text; it shares no code with the library and needs nothing but NumPy.  Test infrastructure only."""
import numpy as np

COUNTS = ("n_tracks", "n_obs", "n_components", "n_short", "n_conflicting", "n_conflicting_nodes", "n_oversize", "n_oversize_nodes",
          "n_singletons")  # (n_rounds is the device's own: the reference has no rounds to compare)


def labels(n_nodes, edges):
    """label (n_nodes,): the smallest node id of every node's component.  Each pass gives both ends of every edge the smaller of
    their two labels, then replaces every label by its label's label until that changes nothing; the passes end when one changes
    no label."""
    label = np.arange(n_nodes, dtype=np.int64)
    u, v = edges[:, 0].astype(np.int64), edges[:, 1].astype(np.int64)
    while True:
        low = np.minimum(label[u], label[v])
        new = label.copy()
        np.minimum.at(new, u, low)
        np.minimum.at(new, v, low)
        while True:
            nxt = new[new]
            if (nxt == new).all():
                break
            new = nxt
        if (new == label).all():
            return label
        label = new


def build_tracks(kp_ptr, kp_xy, edges, edge_ok=None, min_length=2):
    """The dict of lib._mvba.build_tracks without its timings and rounds."""
    kp_ptr = np.asarray(kp_ptr, np.int64)
    m, n = len(kp_ptr) - 1, int(kp_ptr[-1])
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    if edge_ok is not None:
        edges = edges[np.asarray(edge_ok) != 0]
    label = labels(n, edges)
    image = np.searchsorted(kp_ptr, np.arange(n), side="right") - 1  # (the last image whose first node is <= the node)
    size = np.bincount(label, minlength=n)
    roots = np.nonzero(size)[0]
    single, short = size == 1, (size > 1) & (size < min_length)
    over = (size > 1) & ~short & (size > m)
    cand = (size > 1) & ~short & ~over
    # a candidate's nodes in ascending order; two of them in one image: conflicting
    order = np.lexsort((np.arange(n), label))
    order = order[cand[label[order]]]
    same = (label[order][1:] == label[order][:-1]) & (image[order][1:] == image[order][:-1])
    conflict = np.zeros(n, bool)
    conflict[label[order][1:][same]] = True
    keep = cand & ~conflict
    kept_roots = np.nonzero(keep)[0]  # ascending: the order of the tracks
    track_of_root = np.full(n, -1, np.int64)
    track_of_root[kept_roots] = np.arange(len(kept_roots))
    obs_node = order[keep[label[order]]]
    node_track = np.where(single[label], -1, np.where(short[label], -2, np.where(keep[label], track_of_root[label], -3)))
    out = {"pt_ptr": np.concatenate([[0], np.cumsum(size[kept_roots])]).astype(np.int64), "cam_idx": image[obs_node].astype(np.int32),
           "obs_node": obs_node.astype(np.int32), "xy": None if kp_xy is None else np.asarray(kp_xy, np.float64).reshape(-1, 2)[obs_node],
           "node_track": node_track.astype(np.int32), "label": label}
    out.update(n_tracks=len(kept_roots), n_obs=len(obs_node), n_components=int((size[roots] > 1).sum()), n_short=int(short.sum()),
               n_conflicting=int(conflict.sum()), n_conflicting_nodes=int(size[conflict].sum()), n_oversize=int(over.sum()),
               n_oversize_nodes=int(size[over].sum()), n_singletons=int(single.sum()))
    return out
