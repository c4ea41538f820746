"""Pretraining on a user's own molecules at graph-replay speed: a flat molecule store, held in device memory, that feeds
the captured capacity-bucket step (moleculesde_amd/bucket.py) with no per-batch host work.

The reference does this work once per sample in Molecule3DDataset.get (Geom3D/datasets/dataset_3D.py:106-124: slice the
collated arrays, extend_graph, subtract the centre) and lets DataLoader(shuffle=True) collate.  Here:
  * `MoleculeStore` (host): the collated arrays of the whole dataset, molecule-local bond indices, int64 pointer tables, and
    the extended-edge count of every molecule (what sizes the capacities);
  * `EpochPlan` (host, numpy): the permutation of one epoch, this rank's shard, and per batch exactly what
    bucket.raw_sizes would find on the collated batch -- cumulative sums over the permuted per-molecule arrays;
  * `ResidentDataset`: the store's arrays on the device, the epoch's permutation in a static buffer, a device batch counter,
    and csrc/dataset.hip (msde_dataset_gather_batch), which writes the raw blob of batch `counter` straight into Bucket.raw
    -- centring included -- in the layout and conventions of bucket.pack_raw, bit for bit;
  * `DatasetRunner`: the counterpart of pretrain.StreamRunner -- ONE captured graph {gather, plans, forward, backward, Adam};
    an epoch is a loop of replays.  Batches outside the capacities (the short last batch, a molecule of more than 32 atoms)
    take the exact-size eager step on a host-built plan.
Sub-graph masking (--SSL_masking_ratio; Molecule3DDataset.subgraph, dataset_3D.py:53-104, between extend_graph and the
centring) is a per-molecule keep word: drawn once per epoch for the whole store by msde_dataset_mask_epoch (`bfs_keep` is its
bit-exact host mirror), read by msde_dataset_gather_batch_masked before the centre is formed, and -- because the masked
molecule's extended edges are the WHOLE molecule's restricted to the kept atoms, not what the kept bonds span -- handed to
the device plan builder as ready-made rows (Bucket.ext_in, msde_plan_build_ext).  The captured step itself is the same.
"""
import numpy as np
import torch

from . import _lib, bucket as BK, plan as _plan
from ._torchabi import _p, _stream
from .batch import Batch, MolData, extend_graph_index

FORMAT_VERSION = 1
_FIELDS = ("x", "positions", "edge_index", "edge_attr", "atom_ptr", "bond_ptr", "ext_count")
# bits of the gather's error word (csrc/dataset.hip)
GATHER_ERRORS = {1: "a permutation entry outside [0, M)", 2: "a molecule of more atoms than n_max (or none)",
                 4: "the batch's atoms or bonds exceed the capacity", 8: "fewer than B molecules remain in the epoch",
                 16: "a keep word that is zero or names atoms the molecule does not have"}

# ---- sub-graph masking: host mirror of csrc/dataset.hip (dataset_mask_epoch_kernel) ---------------------------------------
_M64 = (1 << 64) - 1
EPOCH_MIX = 0xD1B54A32D192ED69      # DS_EPOCH_MIX


def _mix64(seed, idx):
    """msde_mix64 (csrc/msde_common.h: the mixer of msde_uniform) on Python integers."""
    z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _keep_count(n, ratio):
    """Atoms dataset_3D.py:56-62 keeps of n: sub_num = int(n * (1 - ratio)) and `while len(idx_sub) <= sub_num` stops at
    sub_num + 1 (the script's off-by-one, kept), capped at n."""
    return min(int(n), int(int(n) * (1 - ratio)) + 1)


def keep_counts(ratio, n_max=BK.PLAN_NMAX):
    """keep_count[n] for n = 0..n_max (int32): the table msde_dataset_mask_epoch reads; Python double arithmetic, on the host."""
    return np.array([_keep_count(n, ratio) for n in range(int(n_max) + 1)], dtype=np.int32)


def _nth_bit(w, j):
    for _ in range(j):
        w &= w - 1
    return (w & -w).bit_length() - 1


def bfs_keep(store, ratio, mask_seed, epoch, molecules=None):
    """The keep words of `molecules` (default: the whole store) for (mask_seed, epoch): Python ints, bit i set = atom i kept.
    Draw d of molecule m: u = mix64(mix64(mask_seed + EPOCH_MIX * (epoch + 1), m), d) >> 40 (24 bits) picks member
    (u * count) >> 24, in ascending atom order, of all atoms (d = 0), of the frontier (unkept atoms one stored bond src -> dst
    from a kept atom) while it is not empty, of all unkept atoms otherwise; keep_count[n] draws.  Integers only: equal to
    msde_dataset_mask_epoch bit for bit for molecules of <= 32 atoms, and defined the same way for larger ones."""
    ids = range(len(store)) if molecules is None else [int(i) for i in molecules]
    seed_e = (int(mask_seed) + EPOCH_MIX * (int(epoch) + 1)) & _M64
    ei = store.edge_index.numpy()
    out = []
    for m in ids:
        a0, a1, b0, b1 = store._span(m)
        n = a1 - a0
        rows = [0] * n
        for s_, d_ in zip(ei[0, b0:b1].tolist(), ei[1, b0:b1].tolist()):
            rows[s_] |= 1 << d_
        key, full, kept, frontier = _mix64(seed_e, m), (1 << n) - 1, 0, 0
        for d in range(_keep_count(n, ratio)):
            pool = frontier or (full & ~kept)
            pick = _nth_bit(pool, ((_mix64(key, d) >> 40) * bin(pool).count("1")) >> 24)
            kept |= 1 << pick
            frontier = (frontier | rows[pick]) & ~kept
        out.append(kept)
    return out


def _kept_atoms(keep, n):
    """Ascending atom indices of a keep word (int) or a boolean row of length n."""
    if isinstance(keep, (int, np.integer)):
        keep = int(keep)
        if keep <= 0 or keep >> n:
            raise ValueError(f"keep word {keep:#x} for a molecule of {n} atoms")
        return [i for i in range(n) if (keep >> i) & 1]
    row = np.asarray(torch.as_tensor(keep).cpu().numpy(), dtype=bool).reshape(-1)
    if len(row) != n or not row.any():
        raise ValueError(f"keep row of {len(row)} entries ({int(row.sum())} set) for a molecule of {n} atoms")
    return np.nonzero(row)[0].tolist()


def ext_rows_of(b):
    """Per atom of a collated batch the bit mask of its extended neighbours in molecule-local numbering (int32 [N], the
    contents of Bucket.ext_in), from b.extended_edge_index."""
    first = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(b.batch, minlength=b.num_graphs).cumsum(0)])[b.batch]
    src, dst = b.extended_edge_index
    rows = np.zeros(b.x.size(0), dtype=np.uint32)
    np.bitwise_or.at(rows, src.numpy(), (np.uint32(1) << (dst - first[src]).numpy().astype(np.uint32)))
    return torch.from_numpy(rows.view(np.int32))


def _ext_counts(edge_index, atom_ptr, bond_ptr):
    """Extended edges per molecule (batch.extend_graph_index: ordered pairs within <= 4 bonds), molecules of one size at a
    time as batched boolean matrix powers."""
    n = np.diff(atom_ptr)
    M = len(n)
    out = np.zeros(M, dtype=np.int32)
    bmol = np.repeat(np.arange(M), np.diff(bond_ptr))
    for size in np.unique(n):
        size = int(size)
        if size < 2:
            continue
        ids = np.nonzero(n == size)[0]
        slot = np.full(M, -1, dtype=np.int64)
        step = max(1, (1 << 22) // (size * size))
        for lo in range(0, len(ids), step):
            grp = ids[lo:lo + step]
            slot[:] = -1
            slot[grp] = np.arange(len(grp))
            sel = slot[bmol] >= 0
            A = np.zeros((len(grp), size, size), dtype=bool)
            A[slot[bmol[sel]], edge_index[0, sel], edge_index[1, sel]] = True
            eye = np.eye(size, dtype=bool)[None]
            for _ in range(2):
                Pw = np.matmul(A.astype(np.float32), A.astype(np.float32)) > 0
                A = A | (Pw & ~eye)
            out[grp] = A.reshape(len(grp), -1).sum(1)
    return out


class MoleculeStore:
    """A dataset as flat arrays: x [N, 9] int32, positions [N, 3] float32 (NOT centred), edge_index [2, E] int32
    (molecule-local, directed, stored order), edge_attr [E, 3] int32, atom_ptr / bond_ptr [M + 1] int64, ext_count [M] int32."""

    def __init__(self, x, positions, edge_index, edge_attr, atom_ptr, bond_ptr, ext_count=None):
        t = torch.as_tensor
        self.x = t(x).to(torch.int32).reshape(-1, BK.K_ATOM).contiguous()
        self.positions = t(positions).to(torch.float32).reshape(-1, 3).contiguous()
        self.edge_index = t(edge_index).to(torch.int32).reshape(2, -1).contiguous()
        self.edge_attr = t(edge_attr).to(torch.int32).reshape(-1, 3).contiguous()
        self.atom_ptr = t(atom_ptr).to(torch.int64).reshape(-1).contiguous()
        self.bond_ptr = t(bond_ptr).to(torch.int64).reshape(-1).contiguous()
        self._validate()
        if ext_count is None:
            ext_count = _ext_counts(self.edge_index.numpy(), self.atom_ptr.numpy(), self.bond_ptr.numpy())
        self.ext_count = t(ext_count).to(torch.int32).reshape(-1).contiguous()
        if self.ext_count.numel() != len(self):
            raise ValueError(f"ext_count holds {self.ext_count.numel()} entries for {len(self)} molecules")

    def __len__(self):
        return self.atom_ptr.numel() - 1

    # -- validation ------------------------------------------------------------------------------------------------
    def _validate(self):
        ap, bp = self.atom_ptr.numpy(), self.bond_ptr.numpy()
        N, E = self.x.size(0), self.edge_index.size(1)
        if len(ap) < 2 or len(ap) != len(bp):
            raise ValueError(f"pointer tables of {len(ap)} and {len(bp)} entries: both hold molecules + 1, at least 2")
        if self.positions.size(0) != N or self.edge_attr.size(0) != E:
            raise ValueError(f"x {N} rows vs positions {self.positions.size(0)}; edge_index {E} columns vs edge_attr "
                             f"{self.edge_attr.size(0)} rows")
        for name, ptr, total in (("atom_ptr", ap, N), ("bond_ptr", bp, E)):
            d = np.diff(ptr)
            if (d < 0).any():
                raise ValueError(f"{name} is not monotone at molecule {int(np.nonzero(d < 0)[0][0])}")
            if ptr[0] != 0 or ptr[-1] != total:
                raise ValueError(f"{name} spans [{int(ptr[0])}, {int(ptr[-1])}], the arrays hold {total} rows")
        n = np.diff(ap)
        if (n == 0).any():
            raise ValueError(f"molecule {int(np.nonzero(n == 0)[0][0])} is empty")
        mol_of_atom = lambda rows: int(np.searchsorted(ap, rows[0], side="right") - 1)
        x = self.x.numpy()
        bad = ((x < 0) | (x >= np.asarray(_plan.ATOM_FEATURE_DIMS)[None])).any(1)
        if bad.any():
            raise ValueError(f"molecule {mol_of_atom(np.nonzero(bad)[0])}: an atom feature code outside "
                             f"{_plan.ATOM_FEATURE_DIMS}")
        pos = self.positions.numpy()
        bad = ~np.isfinite(pos).all(1)
        if bad.any():
            raise ValueError(f"molecule {mol_of_atom(np.nonzero(bad)[0])}: a coordinate that is not finite")
        mol_of_bond = lambda rows: int(np.searchsorted(bp, rows[0], side="right") - 1)
        ea = self.edge_attr.numpy()
        bad = ((ea < 0) | (ea >= np.asarray(_plan.BOND_FEATURE_DIMS)[None])).any(1)
        if bad.any():
            raise ValueError(f"molecule {mol_of_bond(np.nonzero(bad)[0])}: a bond feature code outside "
                             f"{_plan.BOND_FEATURE_DIMS}")
        ei = self.edge_index.numpy()
        n_of_bond = np.repeat(n, np.diff(bp))
        bad = ((ei < 0) | (ei >= n_of_bond[None])).any(0)
        if bad.any():
            raise ValueError(f"molecule {mol_of_bond(np.nonzero(bad)[0])}: a bond endpoint outside the molecule")

    # -- constructors and I/O --------------------------------------------------------------------------------------
    @staticmethod
    def from_molecules(mols):
        """From MolData-like objects (x [n, 9], edge_index [2, e] molecule-local, edge_attr [e, 3], positions [n, 3])."""
        mols = list(mols)
        if not mols:
            raise ValueError("no molecules")
        for i, m in enumerate(mols):
            if m.x.dim() != 2 or m.x.size(0) == 0:
                raise ValueError(f"molecule {i} is empty" if m.x.numel() == 0 else f"molecule {i}: x is not [n, {BK.K_ATOM}]")
        cat = lambda ts, d: torch.cat([torch.as_tensor(v) for v in ts], dim=d)
        na = torch.tensor([m.x.size(0) for m in mols], dtype=torch.int64)
        nb = torch.tensor([m.edge_index.reshape(2, -1).size(1) for m in mols], dtype=torch.int64)
        zero = torch.zeros(1, dtype=torch.int64)
        return MoleculeStore(cat([m.x for m in mols], 0), cat([m.positions for m in mols], 0),
                             cat([m.edge_index.reshape(2, -1) for m in mols], 1),
                             cat([m.edge_attr.reshape(-1, 3) for m in mols], 0),
                             torch.cat([zero, na.cumsum(0)]), torch.cat([zero, nb.cumsum(0)]))

    @staticmethod
    def from_collated(data, slices):
        """From the two mappings of an InMemoryDataset's processed file (`geometric_data_processed.pt`: collated tensors and
        their per-key slice tables), read duck-typed: x, edge_index (molecule-local, as InMemoryDataset stores it),
        edge_attr, positions."""
        for k in ("x", "edge_index", "edge_attr", "positions"):
            if k not in data or k not in slices:
                raise ValueError(f"the collated pair has no '{k}'")
        ap, bp = torch.as_tensor(slices["x"]).to(torch.int64), torch.as_tensor(slices["edge_index"]).to(torch.int64)
        if not torch.equal(torch.as_tensor(slices["positions"]).to(torch.int64), ap):
            raise ValueError("slices['positions'] differs from slices['x']")
        if not torch.equal(torch.as_tensor(slices["edge_attr"]).to(torch.int64), bp):
            raise ValueError("slices['edge_attr'] differs from slices['edge_index']")
        return MoleculeStore(data["x"], data["positions"], data["edge_index"], data["edge_attr"], ap, bp)

    def save(self, path):
        d = {k: getattr(self, k) for k in _FIELDS}
        d["format_version"] = FORMAT_VERSION
        torch.save(d, path)

    @staticmethod
    def load(path):
        d = torch.load(path, map_location="cpu", weights_only=True)
        if d.get("format_version") != FORMAT_VERSION:
            raise ValueError(f"{path}: format version {d.get('format_version')}, this build reads {FORMAT_VERSION}")
        return MoleculeStore(*(d[k] for k in _FIELDS))

    # -- per-molecule views ------------------------------------------------------------------------------------------
    def _span(self, i):
        i = int(i)
        if not 0 <= i < len(self):
            raise IndexError(f"molecule {i} of {len(self)}")
        return (int(self.atom_ptr[i]), int(self.atom_ptr[i + 1]), int(self.bond_ptr[i]), int(self.bond_ptr[i + 1]))

    def centred_positions(self, i):
        """dataset_3D.py:120-122 with the arithmetic of csrc/dataset.hip, so that the two agree bit for bit: per axis the
        coordinates are summed in atom order in fp64, divided by n in fp64, rounded to fp32 and subtracted in fp32."""
        a0, a1, _, _ = self._span(i)
        return self._centred(self.positions[a0:a1].numpy())

    @staticmethod
    def _centred(p):
        s = np.zeros(3, dtype=np.float64)
        for row in p:                           # (sequential on purpose: numpy's own sum is pairwise)
            s = s + row.astype(np.float64)
        centre = (s / np.float64(len(p))).astype(np.float32)
        return torch.from_numpy(p - centre[None])

    def molecule(self, i, remove_center=False, extended=False, keep=None):
        """Molecule i as a MolData with int64 fields, as the models and Batch.from_data_list expect; `extended` attaches
        extended_edge_index (dataset_3D.py:116-118), `remove_center` the centred coordinates.  `keep` (a keep word as an int,
        or a boolean row) is the sub-graph of dataset_3D.py:72-102: kept atoms in ascending order, the bonds with both ends
        kept in stored order with relabelled ends, extended_edge_index built on the WHOLE molecule and then filtered the same
        way (two kept atoms joined only through a dropped one stay extended neighbours), the centre over the kept atoms."""
        a0, a1, b0, b1 = self._span(i)
        n = a1 - a0
        ei = self.edge_index[:, b0:b1].to(torch.int64)
        if keep is None:
            d = MolData(x=self.x[a0:a1].to(torch.int64), edge_index=ei, edge_attr=self.edge_attr[b0:b1].to(torch.int64),
                        positions=self.centred_positions(i) if remove_center else self.positions[a0:a1].clone())
            if extended:
                d.extended_edge_index = extend_graph_index(ei, n)
            return d
        idx = torch.tensor(_kept_atoms(keep, n), dtype=torch.int64)
        new = torch.full((n,), -1, dtype=torch.int64)
        new[idx] = torch.arange(idx.numel())

        def induced(e):                          # (torch_geometric.utils.subgraph with relabel_nodes=True)
            sel = (new[e[0]] >= 0) & (new[e[1]] >= 0)
            return new[e[:, sel]], sel
        ei_k, sel = induced(ei)
        pos = self.positions[a0:a1][idx]
        d = MolData(x=self.x[a0:a1][idx].to(torch.int64), edge_index=ei_k, edge_attr=self.edge_attr[b0:b1][sel].to(torch.int64),
                    positions=self._centred(pos.numpy()) if remove_center else pos.clone())
        if extended:
            d.extended_edge_index = induced(extend_graph_index(ei, n))[0]
        return d

    def collate(self, indices, remove_center=True, keeps=None):
        """The host batch of these molecules, in this order (what the reference's loader would collate); `keeps`: one keep
        word (or boolean row) per molecule."""
        keeps = [None] * len(indices) if keeps is None else list(keeps)
        if len(keeps) != len(indices):
            raise ValueError(f"{len(keeps)} keep words for {len(indices)} molecules")
        return Batch.from_data_list([self.molecule(int(i), remove_center=remove_center, extended=True, keep=k)
                                     for i, k in zip(indices, keeps)])

    def epoch_plan(self, epoch, batch_size, shuffle=True, seed=0, rank=0, world=1, perm=None, mask_ratio=0, mask_seed=0):
        return EpochPlan(self, epoch, batch_size, shuffle=shuffle, seed=seed, rank=rank, world=world, perm=perm,
                         mask_ratio=mask_ratio, mask_seed=mask_seed)


class EpochPlan:
    """One epoch on one rank, host only.  The permutation comes from a CPU torch.Generator seeded by (seed, epoch): the same
    on every rank; the rank's shard is perm[rank::world] cut to the common length.  `needs[key][k]` is what bucket.raw_sizes
    finds on the collated batch k (B, N, E_b, E_e from ext_count, E_r = sum n min(n - 1, 32), P = sum n^2, n_max); the short
    last batch is kept (drop_last=False, the DataLoader default the reference uses).
    With mask_ratio > 0 the epoch is one of masked molecules (keep words: bfs_keep(store, mask_ratio, mask_seed, epoch)).  The
    kept atom count depends on n alone, so needs["N"], ["P"] and ["E_r"] are EXACT (from keep_count[n]); needs["E_b"] and
    ["E_e"] stay the unmasked counts -- UPPER BOUNDS (which bonds survive depends on the draw), so `fits` is a sufficient
    condition; needs["n_max"] stays the unmasked size: the keep word is 32 bits, a molecule of more than 32 atoms takes the
    fallback even where its masked size would fit."""

    def __init__(self, store, epoch, batch_size, shuffle=True, seed=0, rank=0, world=1, perm=None, mask_ratio=0, mask_seed=0):
        M, B = len(store), int(batch_size)
        if B < 1 or not 0 <= int(rank) < int(world):
            raise ValueError(f"batch_size {B}, rank {rank} of {world}")
        if not 0 <= float(mask_ratio) < 1:
            raise ValueError(f"mask_ratio {mask_ratio}: outside [0, 1)")
        self.store, self.mask_ratio, self.mask_seed = store, float(mask_ratio), int(mask_seed)
        if perm is not None:
            full = np.asarray(torch.as_tensor(perm).cpu().numpy(), dtype=np.int64).reshape(-1)
            if len(full) and (full.min() < 0 or full.max() >= M):
                first = int(np.nonzero((full < 0) | (full >= M))[0][0])
                raise ValueError(f"permutation entry {first} is {int(full[first])}: outside [0, {M})")
        elif shuffle:
            g = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) & 0x7FFFFFFFFFFFFFFF)
            full = torch.randperm(M, generator=g).numpy()
        else:
            full = np.arange(M, dtype=np.int64)
        self.epoch, self.batch_size, self.rank, self.world = int(epoch), B, int(rank), int(world)
        self.full_perm = full
        self.perm = np.ascontiguousarray(full[rank::world][:len(full) // world])
        L = len(self.perm)
        if L == 0:
            raise ValueError(f"{len(full)} molecules over {world} ranks leave this rank none")
        self.n_batches, self.n_full = -(-L // B), L // B
        n_all = np.diff(store.atom_ptr.numpy())[self.perm]
        n = n_all if not self.mask_ratio else keep_counts(self.mask_ratio, int(n_all.max())).astype(np.int64)[n_all]
        per_mol = {"N": n, "E_b": np.diff(store.bond_ptr.numpy())[self.perm], "E_e": store.ext_count.numpy()[self.perm].astype(np.int64),
                   "E_r": n * np.minimum(np.maximum(n - 1, 0), BK.MAX_NBR), "P": n * n}
        starts = np.arange(self.n_batches) * B
        ends = np.minimum(starts + B, L)
        self.needs = {"B": ends - starts, "n_max": np.maximum.reduceat(n_all, starts)}
        for k, v in per_mol.items():
            c = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
            self.needs[k] = c[ends] - c[starts]

    def __len__(self):
        return self.n_batches

    def need(self, k):
        return {key: int(v[k]) for key, v in self.needs.items()}

    def molecules(self, k):
        return self.perm[k * self.batch_size:(k + 1) * self.batch_size]

    def keeps(self, k):
        """The keep words of batch k's molecules (host mirror), None without masking."""
        return bfs_keep(self.store, self.mask_ratio, self.mask_seed, self.epoch, self.molecules(k)) if self.mask_ratio else None

    def collate(self, k, remove_center=True):
        """The host batch k of this epoch, masked where the plan carries a ratio."""
        return self.store.collate(self.molecules(k), remove_center=remove_center, keeps=self.keeps(k))

    def fits(self, caps):
        """Per batch: does it fit these Caps (bucket.Caps.fits, vectorised)?  The short last batch never does."""
        nd = self.needs
        return ((nd["B"] == caps.B) & (nd["N"] <= caps.N) & (nd["E_b"] <= caps.E_b) & (nd["E_e"] <= caps.E_e) &
                (nd["E_r"] <= caps.E_r) & (nd["P"] <= caps.P) & (nd["n_max"] <= min(caps.n_max, BK.PLAN_NMAX)))


def caps_for(plan, n_max=None):
    """The default capacity rule: Caps.covering over the plan's full batches that csrc/plan.hip can build (molecules of up to
    PLAN_NMAX atoms; the others take the fallback)."""
    ks = [k for k in range(plan.n_full) if plan.needs["n_max"][k] <= (n_max or BK.PLAN_NMAX)]
    if not ks:
        raise BK.BucketOverflow(f"no full batch of {plan.batch_size} molecules with every molecule within "
                                f"{n_max or BK.PLAN_NMAX} atoms: nothing for the captured step to run on")
    return BK.Caps.covering([plan.need(k) for k in ks], n_max=n_max)


class ResidentDataset:
    """The store on the device (uploaded once), the epoch's permutation in a static int32 buffer, the device batch counter
    and the gather's own error word (Bucket.err is cleared by every msde_plan_build).  For masked epochs: the whole-molecule
    extended rows (msde_dataset_ext_rows, once, here) and the keep word of every molecule (msde_dataset_mask_epoch, per epoch)."""

    def __init__(self, store, device):
        self.store, self.device = store, torch.device(device)
        if len(store) >= 2 ** 31:
            raise ValueError("the permutation buffer is int32")
        up = lambda t: t.to(self.device).contiguous()
        self.x, self.pos, self.edge_index, self.edge_attr = up(store.x), up(store.positions), up(store.edge_index), up(store.edge_attr)
        self.atom_ptr, self.bond_ptr = up(store.atom_ptr), up(store.bond_ptr)
        self.perm = torch.zeros(len(store), dtype=torch.int32, device=self.device)
        self.counter = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.n_avail = 0
        self._err_host, self._err_event = None, None
        self.mol_rows = torch.zeros(store.x.size(0), dtype=torch.int32, device=self.device)
        self.keep = torch.zeros(len(store), dtype=torch.int32, device=self.device)
        self.keep_count = torch.zeros(BK.PLAN_NMAX + 1, dtype=torch.int32, device=self.device)
        self.masked = False
        _lib.call("msde_dataset_ext_rows", _p(self.edge_index), _p(self.atom_ptr), _p(self.bond_ptr), len(store),
                  self.x.size(0), self.edge_index.size(1), _p(self.mol_rows), _stream())

    def epoch_plan(self, epoch, batch_size, **kw):
        return self.store.epoch_plan(epoch, batch_size, **kw)

    def begin_epoch(self, plan):
        """Per-epoch setup: the permutation into the static buffer (a torch copy) and the counter back to zero, both on the
        current stream.  The shard length is a launch argument of a captured gather: it may not change under a graph."""
        L = len(plan.perm)
        src = torch.from_numpy(plan.perm.astype(np.int32))
        self.perm[:L].copy_(src.pin_memory() if self.device.type == "cuda" else src, non_blocking=True)
        self.counter.zero_()
        self.n_avail = L
        self.masked = bool(plan.mask_ratio)
        if self.masked:
            self.launch_mask(plan.mask_ratio, plan.mask_seed, plan.epoch)

    def launch_mask(self, ratio, mask_seed, epoch):
        """msde_dataset_mask_epoch on the current stream: the keep word of every molecule of the store for (mask_seed, epoch)
        into self.keep (0 for molecules of more than 32 atoms: the host masks those).  Once per epoch, outside the graph."""
        src = torch.from_numpy(keep_counts(ratio))
        self.keep_count.copy_(src.pin_memory() if self.device.type == "cuda" else src, non_blocking=True)
        _lib.call("msde_dataset_mask_epoch", _p(self.edge_index), _p(self.atom_ptr), _p(self.bond_ptr), len(self.store),
                  self.x.size(0), self.edge_index.size(1), int(mask_seed) & _M64, int(epoch), _p(self.keep_count),
                  _p(self.keep), _stream())

    def launch_gather(self, blob, layout, caps, n_max=None, remove_center=True, n_avail=None, perm=None, counter=None, err=None,
                      ext_in=None, keep=None):
        """msde_dataset_gather_batch on the current stream, unchecked on the host (the kernel's own guards hold): batch
        `counter[0]` of `perm` into `blob` (int32 [layout['_total']]), then counter[0] += 1.  With `ext_in` (int32 [caps.N],
        Bucket.ext_in): msde_dataset_gather_batch_masked of the molecules masked by `keep` (default: this epoch's words)."""
        lay = layout
        perm = self.perm if perm is None else perm
        assert perm.dtype == torch.int32 and perm.is_contiguous() and blob.dtype == torch.int32 and blob.is_contiguous()
        n_avail = self.n_avail if n_avail is None else int(n_avail)
        if n_avail > perm.numel() or blob.numel() < lay["_total"]:
            raise ValueError(f"n_avail {n_avail} vs a permutation of {perm.numel()}; blob {blob.numel()} vs {lay['_total']} words")
        common = (_p(self.x), _p(self.pos), _p(self.edge_index), _p(self.edge_attr), _p(self.atom_ptr), _p(self.bond_ptr),
                  len(self.store), self.x.size(0), self.edge_index.size(1), _p(perm),
                  _p(self.counter if counter is None else counter), n_avail, caps.B, caps.N, caps.E_b,
                  int(caps.n_max if n_max is None else n_max), int(bool(remove_center)),
                  *(lay[k][0] for k in ("x", "pos", "bond_src", "bond_dst", "bond_attr", "mol_atoms", "mol_bonds")),
                  lay["_total"])
        tail = (_p(self.err if err is None else err), _stream())
        if ext_in is None:
            _lib.call("msde_dataset_gather_batch", *common, _p(blob), *tail)
            return
        keep = self.keep if keep is None else keep
        assert ext_in.dtype == torch.int32 and ext_in.is_contiguous() and keep.dtype == torch.int32 and keep.is_contiguous()
        if ext_in.numel() < caps.N or keep.numel() < len(self.store):
            raise ValueError(f"ext_in {ext_in.numel()} vs {caps.N} atom rows; keep {keep.numel()} vs {len(self.store)} molecules")
        _lib.call("msde_dataset_gather_batch_masked", *common, _p(keep), _p(self.mol_rows), _p(blob), _p(ext_in), *tail)

    def gather(self, bk, plan, k, remove_center=True):
        """Host-checked gather of batch k of `plan` (after begin_epoch(plan)) into a bucket: refuses, before any launch, a
        batch the plan marks as not fitting the bucket's capacities."""
        if not 0 <= k < plan.n_batches or not bool(plan.fits(bk.caps)[k]):
            raise BK.BucketOverflow(f"batch {k} {plan.need(k) if 0 <= k < plan.n_batches else ''} does not fit the bucket "
                                    f"{bk.caps.as_dict()}")
        if self.masked and bk.ext_in is None:
            raise ValueError("a masked epoch needs a bucket with ext_in (Bucket(..., ext_in=True))")
        self.counter.fill_(k)
        self.launch_gather(bk.raw, bk.layout, bk.caps, remove_center=remove_center, ext_in=bk.ext_in if self.masked else None)

    def poll_error(self):
        """The gather's error word WITHOUT a synchronisation (Bucket.poll_overflow's scheme): the word as it was when the
        previous poll's copy completed, and the next copy queued behind the work submitted so far."""
        if self._err_host is None:
            self._err_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        seen = 0
        if self._err_event is not None:
            self._err_event.synchronize()
            seen = int(self._err_host[0])
        self._err_host.copy_(self.err, non_blocking=True)
        self._err_event = torch.cuda.Event()
        self._err_event.record()
        return seen


def describe_error(bits):
    return "; ".join(v for b, v in GATHER_ERRORS.items() if bits & b) or "none"


class DatasetRunner:
    """pretrain.StreamRunner's surface (ensure_captured / run / fallbacks) on a resident dataset: ONE bucket, ONE captured graph
    {gather of batch `counter` + device-side plans + forward + backward + Adam}; a step is one replay, nothing is copied
    from or packed on the host.  run(plan, steps) takes an EpochPlan where StreamRunner.run takes batches.
    A plan with a mask ratio makes it the masked runner: the graph holds the masked gather and the plan build on Bucket.ext_in,
    every epoch's plan must carry a ratio too (the keep words are redrawn per epoch, outside the graph), and the fallbacks
    collate host-masked molecules of the same (mask_seed, epoch)."""

    def __init__(self, trainer, resident, plan, caps=None, remove_center=True):
        from . import pretrain as PT
        self.PT, self.tr, self.rd, self.remove_center = PT, trainer, resident, bool(remove_center)
        self.caps = caps or caps_for(plan)
        trainer.check_bucket_metric()
        fits = plan.fits(self.caps)
        if not bool(fits[0]):
            raise BK.BucketOverflow(f"the first batch {plan.need(0)} does not fit the bucket {self.caps.as_dict()}")
        self._check_neg_samples(plan)
        self.masked = bool(plan.mask_ratio)
        self.bk = bk = trainer.make_bucket(self.caps)
        if self.masked:
            bk.alloc_ext_in()
        self.fallbacks = 0
        # warm up as Trainer.capture_bucket does: batch 0 gathered eagerly, its plans, two eager steps; then capture
        resident.begin_epoch(plan)
        self.n_avail = resident.n_avail
        self._gather()
        bk.build_plan_on_device()
        ok, sizes = bk.check()
        bits = int(resident.err.cpu())
        if not ok or bits:
            raise BK.BucketOverflow(f"batch does not fit the bucket: {sizes} vs {self.caps.as_dict()} (gather: {describe_error(bits)})")
        for _ in range(2):
            trainer.step(bk.batch)
        self._capture()

    def _gather(self):
        self.rd.launch_gather(self.bk.raw, self.bk.layout, self.caps, remove_center=self.remove_center, n_avail=self.n_avail,
                              ext_in=self.bk.ext_in if self.masked else None)

    def _capture(self):
        tr, PT = self.tr, self.PT
        side = tr._side_stream if (tr.overlap_streams and PT.PLAN_LISTS_ON_SIDE) else None
        tr.capture(self.bk.batch, pre=lambda: (self._gather(), self.bk.build_plan_on_device(side)))
        self._captured_coeffs = (float(tr.coeff_cl),)

    def ensure_captured(self):
        """The loss coefficients are baked into the graph: after a change (contrastive skip epochs) capture again."""
        if (float(self.tr.coeff_cl),) != self._captured_coeffs:
            self.tr.check_bucket_metric()
            # (the superseded graph is parked, not destroyed: see StreamRunner.ensure_captured)
            self._parked = getattr(self, "_parked", []) + [self.tr._graphs.pop(id(self.bk.batch), None)]
            self._capture()

    def _check_neg_samples(self, plan):
        """EBM_dot_prod: 1 <= K < N (pretrain.check_bucket_neg_samples) for the smallest batch of the epoch, before it starts."""
        a = self.tr.args
        if a.CL_similarity_metric == "EBM_dot_prod" and self.tr.coeff_cl > 0:
            self.PT._neg_samples(a, int(plan.needs["N"].min()))

    def run(self, plan, steps=None):
        """One epoch (or its first `steps` batches).  Returns the number of steps taken."""
        n = plan.n_batches if steps is None else min(int(steps), plan.n_batches)
        if n == 0:
            return 0
        if len(plan.perm) != self.n_avail:
            raise ValueError(f"an epoch of {len(plan.perm)} molecules on a graph captured for {self.n_avail}")
        if bool(plan.mask_ratio) != self.masked:
            raise ValueError(f"an epoch with mask_ratio {plan.mask_ratio} on a graph captured {'with' if self.masked else 'without'} masking")
        fits = plan.fits(self.caps)
        self._check_neg_samples(plan)
        rd, bk, tr = self.rd, self.bk, self.tr
        rd.begin_epoch(plan)
        for k in range(n):
            if fits[k]:
                bits = rd.poll_error()
                if bits or bk.poll_overflow():
                    raise BK.BucketOverflow(f"a batch did not fit the bucket {self.caps.as_dict()} (gather: {describe_error(bits)}): "
                                            "that step is not a valid update")
                tr.step_graph(bk.batch)
            else:                               # exact-size eager step on a host-built plan; the device counter moves on
                self.fallbacks += 1
                tr.step(self.PT.prepare_batch(plan.collate(k, remove_center=self.remove_center), tr.device))
                rd.counter.add_(1)
        return n


class EagerDatasetRunner:
    """The exact-size loop over host-collated batches of the same epoch plans (pretrain --eager --dataset_file).
    `start_plan`: take DatasetRunner's start on that plan -- its two warm-up updates on the plan's first batch, then every
    draw seeded by the device step counter as Trainer.capture arranges for a captured step -- so that this loop is the eager
    twin of the replayed run: same updates, same draws, same epoch losses.  pretrain.main asks for it under
    --SSL_masking_ratio, where the two modes of one command are meant to agree; without it the loop starts as it always did."""
    fallbacks = 0

    def __init__(self, trainer, store, remove_center=True, start_plan=None):
        self.tr, self.store, self.remove_center = trainer, store, bool(remove_center)
        if start_plan is not None:
            from .geom3d import prepare_batch
            b = prepare_batch(start_plan.collate(0, remove_center=self.remove_center), trainer.device)
            for _ in range(2):
                trainer.step(b)
            sd = trainer.step_counter.view(torch.int64)
            trainer.models["SDE_2Dto3D_model"].score_network.seed_dev = sd
            if hasattr(trainer.noise, "seed_dev"):
                trainer.noise.seed_dev = sd

    def ensure_captured(self):
        pass

    def run(self, plan, steps=None):
        from .geom3d import prepare_batch
        n = plan.n_batches if steps is None else min(int(steps), plan.n_batches)
        for k in range(n):
            self.tr.step(prepare_batch(plan.collate(k, remove_center=self.remove_center), self.tr.device))
        return n
