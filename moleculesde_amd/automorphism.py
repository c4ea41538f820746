"""Graph automorphisms of a molecule on the host, for the symmetry-aware conformer evaluation (conformer_eval.py).

Pure Python / NumPy: colour refinement (1-dimensional Weisfeiler-Leman on atom and bond colours) to cut the candidates, then
a backtracking search that maps the atoms in breadth-first order, so that every atom but the first of a connected component
is mapped next to an already mapped neighbour.  A molecule of at most a few hundred atoms takes milliseconds, once per
molecule.  What is matched is what rdkit's `GetBestRMS` matches on: element and bond order, no chirality."""
import numpy as np


def _graph(n, edge_index, bond_colour, keep):
    """adj[u] = {v: bond colour} of the sub-graph induced by the kept atoms, undirected.  Self-loops and bonds with a dropped
    end are left out; a bond stored once, twice or more is one bond (with the smallest of its colours)."""
    adj = [dict() for _ in range(n)]
    ei = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    bc = np.asarray(bond_colour, dtype=np.int64).reshape(-1)
    if bc.size != ei.shape[1]:
        raise ValueError(f"{bc.size} bond colours for {ei.shape[1]} bonds")
    if ei.size and (ei.min() < 0 or ei.max() >= n):
        raise ValueError(f"edge_index names atoms outside [0, {n})")
    for u, v, c in zip(ei[0].tolist(), ei[1].tolist(), bc.tolist()):
        if u == v or not (keep[u] and keep[v]):
            continue
        c = min(c, adj[u].get(v, c))
        adj[u][v] = c
        adj[v][u] = c
    return adj


def _refine(atoms, adj, colour):
    """Stable colouring: atoms of one class have the same colour and the same multiset of (bond colour, neighbour class)."""
    cls = {a: colour[a] for a in atoms}
    count = len(set(cls.values()))
    while True:
        sig = {a: (cls[a], tuple(sorted((c, cls[v]) for v, c in adj[a].items()))) for a in atoms}
        ids = {s: i for i, s in enumerate(sorted(set(sig.values())))}
        cls = {a: ids[sig[a]] for a in atoms}
        if len(ids) == count:
            return cls
        count = len(ids)


def automorphisms(n, edge_index, atom_colour, bond_colour, keep=None, max_count=1024):
    """The colour-preserving automorphisms of the sub-graph induced by the kept atoms: (perms [P, n] int32, truncated).

    n atoms; edge_index [2, E] (both directions, as the records store it; one direction only, duplicates and self-loops are
    tolerated, bonds with a dropped end ignored); atom_colour [n] (x[:, 0], the atomic number minus one); bond_colour [E]
    (edge_attr[:, 0], the bond type); keep [n] bool or None (all atoms).  The kept sub-graph may be disconnected: identical
    components may swap.

    perms[p][a] is the atom that atom a is mapped to -- in conformer_eval, the REFERENCE atom compared with atom a of the
    generated conformer.  Every row is a bijection of the kept atoms onto the kept atoms that preserves both colourings and
    adjacency; dropped atoms map to themselves.  perms[0] is the identity and the order is deterministic: lexicographic in
    the search order (atoms breadth-first from the lowest index, candidates ascending).

    max_count: the enumeration stops there and returns truncated = True when the group is larger.  A truncated set still
    holds the identity, so a best RMSD over it is still an upper bound of the true one and never worse than plain Kabsch.
    The default of 1024 is a MEMORY bound on the table (P n int32 per molecule), not a measured figure; rdkit's own cap
    (`maxMatches` of GetBestRMS) is 10^6 matches."""
    n = int(n)
    max_count = int(max_count)
    if max_count < 1:
        raise ValueError("max_count must be at least 1")
    colour = np.asarray(atom_colour, dtype=np.int64).reshape(-1)
    if colour.size != n:
        raise ValueError(f"{colour.size} atom colours for {n} atoms")
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    if keep.size != n:
        raise ValueError(f"keep has {keep.size} entries for {n} atoms")
    keep = keep.tolist()
    atoms = [a for a in range(n) if keep[a]]
    adj = _graph(n, edge_index, bond_colour, keep)
    cls = _refine(atoms, adj, colour.tolist())
    members = {}
    for a in atoms:
        members.setdefault(cls[a], []).append(a)

    # search order: breadth-first from the lowest unvisited atom, neighbours ascending; parent[a] = the neighbour it was
    # reached from (None for the first atom of a component), earlier[a] = its neighbours that come before it in the order
    order, parent, pos = [], {}, {}
    for root in atoms:
        if root in pos:
            continue
        pos[root], parent[root] = len(order), None
        order.append(root)
        head = len(order) - 1
        while head < len(order):
            u = order[head]
            head += 1
            for v in sorted(adj[u]):
                if v not in pos:
                    pos[v], parent[v] = len(order), u
                    order.append(v)
    earlier = {a: [(b, c) for b, c in adj[a].items() if pos[b] < pos[a]] for a in atoms}

    def candidates(a, image):
        b = parent[a]
        if b is None:
            return members[cls[a]]
        want = adj[a][b]
        return sorted(v for v, c in adj[image[b]].items() if c == want and cls[v] == cls[a])

    # Iterative depth-first search.  An atom's class fixes its degree, so a bijection that carries every bond onto a bond of
    # the same colour carries non-bonds onto non-bonds: checking each bond once, when its later end is placed, is enough.
    out, truncated = [], False
    image, used = {}, set()
    stack = [iter(candidates(order[0], image))] if order else []
    if not order:
        out.append(list(range(n)))
    while stack:
        depth = len(stack) - 1
        a = order[depth]
        if a in image:                                   # back at this depth: undo the choice made before
            used.discard(image.pop(a))
        placed = False
        for v in stack[-1]:
            if v in used or any(adj[v].get(image[b]) != c for b, c in earlier[a]):
                continue
            image[a] = v
            used.add(v)
            placed = True
            break
        if not placed:
            stack.pop()
            continue
        if depth + 1 == len(order):
            if len(out) == max_count:
                truncated = True
                break
            row = list(range(n))
            for u, v in image.items():
                row[u] = v
            out.append(row)
        else:
            stack.append(iter(candidates(order[depth + 1], image)))
    return np.asarray(out, dtype=np.int32).reshape(len(out), n), truncated
