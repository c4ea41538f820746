"""Sub-graph masking on the device-resident molecule store (--SSL_masking_ratio; csrc/dataset.hip, csrc/plan.hip
msde_plan_build_ext, moleculesde_amd/dataset.py).

1. msde_dataset_mask_epoch words == bfs_keep (the integer host mirror), the 32-atom molecules included.
2. msde_dataset_ext_rows == the rows of extend_graph_index on each whole molecule.
3. The masked gather's blob == pack_raw(store.collate(mols, keeps=...)) word for word, ext_in == the host rows.
4. msde_plan_build_ext on that bucket == the host plan of the host-masked batch; for the path of 6 atoms with atom 1 dropped
   it differs from what msde_plan_build derives from the same blob (the induced extended edges).
5. Guards.  6. DatasetRunner replays == the eager twin.  7. The short last batch.  8. pretrain.main (two tests).
9. The masked and the unmasked gather are two forms of one kernel: with full keep words the blobs are equal bit for bit, and
   the guards they share raise the same bits through either entry point.
"""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dataset_cases import capturable_noise, off_centre_molecules  # noqa: E402
from dataset_mask_cases import B, PATH6, bits, mask_store  # noqa: E402
from helpers import disable_dropout  # noqa: E402

RATIOS = (0.15, 0.5, 0.97)
PATH6_KEEP = 0b111101            # atoms {0, 2, 3, 4, 5}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _collect_graphs_and_buckets_here():
    """(tests/test_gpu_dataset.py: buckets and trainers with captured graphs are collected with the device idle)"""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _words(t):
    return [int(w) & 0xFFFFFFFF for w in t.cpu().tolist()]


@pytest.fixture(scope="module")
def case(dev):
    """The 40-molecule store, its resident copy, the UNMASKED plan of epoch 1 and its capacities (masked batches are smaller:
    they always fit), computed once."""
    from moleculesde_amd import bucket as BK
    from moleculesde_amd.dataset import ResidentDataset, caps_for
    store = mask_store()
    whole = store.epoch_plan(1, B, seed=3)
    caps = caps_for(whole)
    assert whole.n_batches == whole.n_full == 5 and caps.n_max == 32
    return types.SimpleNamespace(store=store, whole=whole, caps=caps, BK=BK, rd=ResidentDataset(store, dev),
                                 n=np.diff(store.atom_ptr.numpy()))


def test_mask_epoch_words_equal_the_host_mirror(dev, case):
    from moleculesde_amd.dataset import bfs_keep, keep_counts
    rd, store = case.rd, case.store
    assert 32 in case.n.tolist() and 1 in case.n.tolist()
    seen = set()
    for r in RATIOS:
        for epoch in (1, 2):
            rd.launch_mask(r, 11, epoch)
            got = _words(rd.keep)
            want = bfs_keep(store, r, 11, epoch)
            assert got == want, (r, epoch, [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w][:4])
            assert all(bin(w).count("1") == keep_counts(r)[n] for w, n in zip(got, case.n))
            seen.add(tuple(got))
    assert len(seen) == 6
    rd.launch_mask(0.01, 11, 1)                                      # every atom kept: full-width words, n = 32 included
    assert _words(rd.keep) == [(1 << int(n)) - 1 for n in case.n]


def test_ext_rows_equal_extend_graph_of_each_whole_molecule(dev, case):
    from moleculesde_amd.batch import extend_graph_index
    store, got = case.store, _words(case.rd.mol_rows)
    want = []
    for i in range(len(store)):
        m = store.molecule(i)
        rows = [0] * m.x.size(0)
        for s, d in extend_graph_index(m.edge_index, m.x.size(0)).t().tolist():
            rows[s] |= 1 << d
        want += rows
    assert got == want
    assert any(w >> 31 for w in want)                                # a 32-atom molecule reaches its last atom


def _masked_bucket(case, dev):
    bk = case.BK.Bucket(case.caps, dev, ext_in=True)
    bk.raw.fill_(-1)                                                 # stale contents everywhere
    bk.ext_in.fill_(-1)
    return bk


def _gather_masked(case, bk, plan, k, keep_dev=None, remove_center=True):
    rd = case.rd
    rd.counter.fill_(k)
    rd.launch_gather(bk.raw, bk.layout, case.caps, remove_center=remove_center, ext_in=bk.ext_in, keep=keep_dev)
    torch.cuda.synchronize()
    assert int(rd.counter.cpu()) == k + 1 and int(rd.err.cpu()) == 0


def _check_blob(case, bk, mols, keeps, remove_center=True):
    from moleculesde_amd.dataset import ext_rows_of
    host = case.store.collate(mols, remove_center=remove_center, keeps=keeps)
    want = case.BK.pack_raw(host, case.caps)
    got = bk.raw.cpu()
    diff = (got != want).nonzero().flatten()
    assert diff.numel() == 0, (diff[:8].tolist(), dict(bk.layout))
    rows = ext_rows_of(host)
    N = host.x.size(0)
    assert torch.equal(bk.ext_in[:N].cpu(), rows) and not bool(bk.ext_in[N:].any())
    return host


def _injected(case, plan):
    """Keep words for the whole store: the path of 6 without atom 1, every atom of the first and of a 32-atom molecule, the
    host mirror's words (ratio 0.5) elsewhere."""
    from moleculesde_amd.dataset import bfs_keep
    keeps = bfs_keep(case.store, 0.5, 4, 9)
    keeps[PATH6] = PATH6_KEEP
    full32 = int(np.nonzero(case.n == 32)[0][0])
    for m in (0, full32):
        keeps[m] = (1 << int(case.n[m])) - 1
    k_path = int(np.nonzero(plan.perm == PATH6)[0][0]) // B
    k_32 = int(np.nonzero(plan.perm == full32)[0][0]) // B
    return keeps, k_path, k_32


def _keep_tensor(keeps, dev):
    return torch.from_numpy(np.array(keeps, dtype=np.uint32).view(np.int32)).to(dev)


@pytest.mark.parametrize("remove_center", [True, False], ids=["centred", "raw"])
def test_masked_gather_blob_equals_pack_raw_of_the_host_masked_batch(dev, case, remove_center):
    rd, whole = case.rd, case.whole
    bk = _masked_bucket(case, dev)
    # (a) the kernel-made keep words of a masked epoch
    plan = case.store.epoch_plan(1, B, seed=3, mask_ratio=0.15, mask_seed=5)
    rd.begin_epoch(plan)
    assert bool(plan.fits(case.caps).all())
    for k in (0, 3):
        _gather_masked(case, bk, plan, k, remove_center=remove_center)
        keeps = plan.keeps(k)
        assert keeps == [_words(rd.keep)[int(m)] for m in plan.molecules(k)]
        host = _check_blob(case, bk, plan.molecules(k), keeps, remove_center)
        assert case.BK.raw_sizes(host)["N"] == plan.need(k)["N"] <= whole.need(k)["N"]
    assert int(plan.needs["N"].sum()) < int(whole.needs["N"].sum())
    # (b) injected keep words
    keeps, k_path, k_32 = _injected(case, whole)
    kd = _keep_tensor(keeps, dev)
    for k in sorted({k_path, k_32}):
        _gather_masked(case, bk, whole, k, keep_dev=kd, remove_center=remove_center)
        _check_blob(case, bk, whole.molecules(k), [keeps[int(m)] for m in whole.molecules(k)], remove_center)


def _full_keeps(case, dev):
    return _keep_tensor([(1 << int(n)) - 1 for n in case.n], dev)


@pytest.mark.parametrize("remove_center", [True, False], ids=["centred", "raw"])
def test_full_keep_words_make_the_masked_gather_the_unmasked_one(dev, case, remove_center):
    """The two forms of dataset_gather_kernel are one algorithm: with every atom kept the masked form writes the unmasked
    form's blob bit for bit, and ext_in is the whole molecules' rows (the compress step is the identity).  Every batch."""
    rd, whole, caps = case.rd, case.whole, case.caps
    rd.begin_epoch(whole)
    a, b = case.BK.Bucket(caps, dev), case.BK.Bucket(caps, dev, ext_in=True)
    full = _full_keeps(case, dev)
    ptr = case.store.atom_ptr.numpy()
    rows = rd.mol_rows.cpu()
    ctr_a, ctr_b = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    err_a, err_b = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
    for k in range(whole.n_batches):
        for t in (a.raw, b.raw, b.ext_in):
            t.fill_(-1)
        rd.launch_gather(a.raw, a.layout, caps, remove_center=remove_center, counter=ctr_a, err=err_a)
        rd.launch_gather(b.raw, b.layout, caps, remove_center=remove_center, counter=ctr_b, err=err_b, ext_in=b.ext_in, keep=full)
        torch.cuda.synchronize()
        assert int(err_a.cpu()) == 0 and int(err_b.cpu()) == 0 and int(ctr_a.cpu()) == k + 1 == int(ctr_b.cpu())
        diff = (a.raw != b.raw).nonzero().flatten()
        assert diff.numel() == 0, (k, diff[:8].tolist(), dict(a.layout))
        assert bool((a.raw != -1).any())
        atoms = torch.from_numpy(np.concatenate([np.arange(ptr[int(m)], ptr[int(m) + 1]) for m in whole.molecules(k)]))
        N = atoms.numel()
        assert N == whole.need(k)["N"] and torch.equal(b.ext_in[:N].cpu(), rows[atoms]), k
        assert not bool(b.ext_in[N:].any())


def test_plan_build_ext_equals_the_host_plan_and_differs_from_the_bond_derived_one(dev, case):
    from test_gpu_plan import _check_plan_equal
    rd, whole = case.rd, case.whole
    bk = _masked_bucket(case, dev)
    rd.begin_epoch(whole)
    keeps, k_path, k_32 = _injected(case, whole)
    kd = _keep_tensor(keeps, dev)
    for k in sorted({k_path, k_32}):
        _gather_masked(case, bk, whole, k, keep_dev=kd)
        host = case.store.collate(whole.molecules(k), keeps=[keeps[int(m)] for m in whole.molecules(k)])
        bk.build_plan_on_device()
        _check_plan_equal(bk, host)                                  # ext.rowptr/src/dst/rowptr_s/perm_s and sizes[2] among them
    # the same blob through msde_plan_build (no ext_in): the extended rows derived from the KEPT bonds miss the pairs joined
    # through the dropped atom -- what the feature corrects.  Every other molecule of the batch keeps all its atoms
    only = [(1 << int(n)) - 1 for n in case.n]
    only[PATH6] = PATH6_KEEP
    _gather_masked(case, bk, whole, k_path, keep_dev=_keep_tensor(only, dev))
    bk.build_plan_on_device()
    torch.cuda.synchronize()
    ee, N = int(bk.sizes[2].cpu()), int(bk.sizes[0].cpu())
    ext = (bk.plan.ext.rowptr[:N + 1].cpu(), bk.plan.ext.src[:ee].cpu(), bk.plan.ext.dst[:ee].cpu())
    plain = case.BK.Bucket(case.caps, dev)
    plain.load(bk.raw)
    plain.build_plan_on_device()
    torch.cuda.synchronize()
    assert plain.check()[0]
    ee_plain = int(plain.sizes[2].cpu())
    assert ee_plain == ee - 6, (ee_plain, ee)                        # (0,1) (0,2) (0,3) of the masked path and their reverses
    assert not torch.equal(plain.plan.ext.rowptr[:N + 1].cpu(), ext[0])
    for name in ("rowptr", "src", "dst"):                            # the bond graph is the same
        assert torch.equal(getattr(plain.plan.bond, name), getattr(bk.plan.bond, name))


def test_guards_bad_keep_words_write_nothing_and_bad_rows_are_sanitised(dev, case):
    rd, whole, caps, BK = case.rd, case.whole, case.caps, case.BK
    rd.begin_epoch(whole)
    lay = BK.raw_layout(caps)
    GUARD, SENT = 64, -0x5A5A5A5B
    good = [(1 << int(n)) - 1 for n in case.n]
    target = next(int(m) for m in whole.molecules(0) if case.n[int(m)] < 32)
    for what, word in (("keep word 0", 0), ("a bit at n", (1 << int(case.n[target])) | 1)):
        buf = torch.full((GUARD + lay["_total"] + GUARD,), SENT, dtype=torch.int32, device=dev)
        ebuf = torch.full((GUARD + caps.N + GUARD,), SENT, dtype=torch.int32, device=dev)
        blob, ext_in = buf[GUARD:GUARD + lay["_total"]], ebuf[GUARD:GUARD + caps.N]
        ctr = torch.ones(1, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err, ext_in=ext_in, keep=_keep_tensor(good, dev))    # a valid batch 1
        before, ebefore = buf.clone(), ebuf.clone()
        assert int(err.cpu()) == 0 and bool((blob != SENT).any()) and bool((ext_in != SENT).all())
        bad = list(good)
        bad[target] = word
        ctr.zero_()
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err, ext_in=ext_in, keep=_keep_tensor(bad, dev))
        torch.cuda.synchronize()
        assert int(err.cpu()) == 16, (what, int(err.cpu()))
        assert torch.equal(buf, before) and torch.equal(ebuf, ebefore), what + ": blob, ext_in and guard bands untouched"
        assert int(ctr.cpu()) == 1
    # msde_plan_build_ext: a row with its self bit (and one at n) raises the bucket's err and is sanitised
    bk = _masked_bucket(case, dev)
    _gather_masked(case, bk, whole, 0, keep_dev=_keep_tensor(good, dev))
    bk.build_plan_on_device()
    ok, sizes = bk.check()
    assert ok
    ref = (bk.plan.ext.rowptr.clone(), bk.plan.ext.src.clone(), bk.plan.ext.dst.clone(), bk.ext_rows.clone())
    clean = bk.ext_in.clone()
    n_first = int(case.n[int(whole.perm[0])])
    assert n_first < 32
    bk.ext_in[0] = bk.ext_in[0] | 1 | (1 << n_first)                 # atom 0 of the first molecule: self bit + a bit at n
    bk.build_plan_on_device()
    torch.cuda.synchronize()
    assert int(bk.err.cpu()) == 1
    assert int(bk.sizes[2].cpu()) == sizes["E_e"] and torch.equal(bk.ext_rows, ref[3])
    assert all(torch.equal(a, b) for a, b in zip((bk.plan.ext.rowptr, bk.plan.ext.src, bk.plan.ext.dst), ref[:3]))
    bk.ext_in.copy_(clean)
    bk.build_plan_on_device()
    torch.cuda.synchronize()
    assert int(bk.err.cpu()) == 0


def test_shared_guards_report_the_same_bits_through_both_entry_points(dev, case):
    """The four argument guards of tests/test_gpu_dataset.py::test_guards_write_nothing_and_set_the_error_word on this store,
    through the masked entry with full keep words: the error word is exactly the bit the unmasked entry raises for the same
    input, blob, ext_in and their guard bands keep the valid previous gather, the counter advances."""
    rd, whole, BK, M = case.rd, case.whole, case.BK, len(case.store)
    rd.begin_epoch(whole)
    atoms = [whole.need(k)["N"] for k in range(5)]
    k_big, k_prev = int(np.argmax(atoms)), int(np.argmin(atoms))
    k32 = next(k for k in range(5) if whole.need(k)["n_max"] == 32)
    assert atoms[k_prev] < atoms[k_big]                              # the previous batch fits the capacity one row short
    tight = types.SimpleNamespace(B=B, N=atoms[k_big] - 1, E_b=case.caps.E_b, n_max=32)
    bad_perm = torch.from_numpy(whole.perm.astype(np.int32)).to(dev)
    bad_perm[3] = M
    full = _full_keeps(case, dev)
    GUARD, SENT = 64, -0x5A5A5A5B
    cases = [("perm entry == M", case.caps, dict(perm=bad_perm), 0, 1),
             ("32 atoms, n_max 24", case.caps, dict(n_max=24), k32, 2),
             ("capacity one row short", tight, dict(), k_big, 4),
             ("fewer than B remain", case.caps, dict(n_avail=B * 5 - 1), 4, 8)]
    for what, caps, kw, k, bit in cases:
        lay = BK.raw_layout(caps)
        buf = torch.full((GUARD + lay["_total"] + GUARD,), SENT, dtype=torch.int32, device=dev)
        ebuf = torch.full((GUARD + caps.N + GUARD,), SENT, dtype=torch.int32, device=dev)
        ubuf = buf.clone()                                           # the unmasked entry's blob
        blob, ext_in, ublob = buf[GUARD:GUARD + lay["_total"]], ebuf[GUARD:GUARD + caps.N], ubuf[GUARD:GUARD + lay["_total"]]
        ctr = torch.full((1,), k_prev, dtype=torch.int32, device=dev)
        err, uerr = (torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2))
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err, ext_in=ext_in, keep=full)         # a valid previous batch
        before, ebefore = buf.clone(), ebuf.clone()
        assert int(err.cpu()) == 0 and bool((blob != SENT).any()) and bool((ext_in != SENT).all())
        uctr = torch.full((1,), k, dtype=torch.int32, device=dev)
        rd.launch_gather(ublob, lay, caps, counter=uctr, err=uerr, **kw)
        ctr.fill_(k)
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err, ext_in=ext_in, keep=full, **kw)
        torch.cuda.synchronize()
        assert int(uerr.cpu()) == bit and int(err.cpu()) == bit, (what, int(uerr.cpu()), int(err.cpu()))
        assert torch.equal(buf, before) and torch.equal(ebuf, ebefore), what + ": blob, ext_in and guard bands untouched"
        for t in (buf, ebuf):
            assert bool((t[:GUARD] == SENT).all()) and bool((t[-GUARD:] == SENT).all()), what
        assert bool((ubuf == SENT).all()), what
        assert int(ctr.cpu()) == k + 1 == int(uctr.cpu())


def _trainer(args, dev, seed):
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    torch.manual_seed(seed)
    tr = pretrain.Trainer(args, dev)
    for m in tr.models.values():
        disable_dropout(m)
    nz = capturable_noise(G, dev)
    tr.noise = nz
    tr.models["SDE_2Dto3D_model"].noise = nz
    return tr


class _EagerTwin:
    """The masked epoch in ONE bucket with every kernel launched from the host: per batch the host-masked blob, the host
    rows into ext_in, the device plan build, Trainer.step."""
    fallbacks = 0

    def __init__(self, tr, caps, plan):
        from moleculesde_amd import bucket as BK
        self.BK, self.tr = BK, tr
        self.bk = tr.make_bucket(caps)
        self.bk.alloc_ext_in()
        self._feed(plan, 0)
        for _ in range(2):                       # DatasetRunner's warm-up: two eager steps on the first batch
            tr.step(self.bk.batch)
        sd = tr.step_counter.view(torch.int64)   # ... and what Trainer.capture then does to the draws: seeded by the step counter
        tr.models["SDE_2Dto3D_model"].score_network.seed_dev = sd
        tr.noise.seed_dev = sd

    def _feed(self, plan, k):
        from moleculesde_amd.dataset import ext_rows_of
        bk, host = self.bk, plan.collate(k)
        bk.load(self.BK.pack_raw(host, bk.caps))
        bk.ext_in.zero_()
        rows = ext_rows_of(host)
        bk.ext_in[:rows.numel()].copy_(rows)
        bk.build_plan_on_device()

    def ensure_captured(self):
        pass

    def run(self, plan, steps=None):
        for k in range(plan.n_batches):
            self._feed(plan, k)
            self.tr.step(self.bk.batch)
        return plan.n_batches


def test_masked_dataset_runner_matches_its_eager_twin(dev):
    """Run A: DatasetRunner replays {masked gather, plan build on ext_in, step}.  Run B: _EagerTwin.  Tolerances: those of
    tests/test_gpu_plan.py::test_stream_runner_matches_its_eager_twin_and_main_runs (a replay against its eager twin)."""
    from moleculesde_amd import bucket as BK, hip, pretrain
    from moleculesde_amd.dataset import DatasetRunner, MoleculeStore, ResidentDataset
    args = pretrain.readme_args(emb_dim=64, SDE_coeff_generative_3Dto2D=0, batch_size=B, epochs=2)
    args.output_model_dir = ""
    sizes = np.random.default_rng(8).integers(2, 25, size=24)
    store = MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=22))
    plans = {e: store.epoch_plan(e, B, seed=1, mask_ratio=0.15, mask_seed=2) for e in (1, 2)}
    caps = BK.Caps.covering([store.epoch_plan(e, B, seed=1).need(k) for e in (1, 2) for k in range(3)], n_max=24)
    quiet = lambda *_: None
    tr = _trainer(args, dev, 11)
    rd = ResidentDataset(store, dev)
    ra = DatasetRunner(tr, rd, plans[1], caps=caps)
    ha = pretrain.train_epochs(args, tr, ra, lambda e: (plans[e], None), out=quiet)
    torch.cuda.synchronize()
    pa = tr.opt.flat_p.clone()
    assert ra.fallbacks == 0 and int(rd.counter.cpu()) == 3 and int(rd.err.cpu()) == 0 and ra.bk.check()[0]
    # two epochs draw different masks: the same permutation forced on both, the first batch's blob differs
    blobs = []
    caps_f = BK.Caps.covering([store.epoch_plan(1, B, perm=np.arange(24)).need(0)], n_max=24)
    bkf = BK.Bucket(caps_f, dev, ext_in=True)
    for e in (1, 2):
        forced = store.epoch_plan(e, B, perm=np.arange(24), mask_ratio=0.15, mask_seed=2)
        rd.begin_epoch(forced)
        rd.gather(bkf, forced, 0)
        blobs.append(bkf.raw.cpu())
        assert torch.equal(blobs[-1], BK.pack_raw(forced.collate(0), caps_f))
    assert not torch.equal(blobs[0], blobs[1])
    hip.clear_row_bounds()
    tr = _trainer(args, dev, 11)
    hb = pretrain.train_epochs(args, tr, _EagerTwin(tr, caps, plans[1]), lambda e: (plans[e], None), out=quiet)
    torch.cuda.synchronize()
    pb = tr.opt.flat_p.clone()
    hip.clear_row_bounds()
    rel = float((pa - pb).norm() / pb.norm())
    print("masked dataset runner vs eager twin:", [e[:4] for e in ha], [e[:4] for e in hb], "params rel", rel)
    assert [e[5] for e in ha] == [3, 3] == [e[5] for e in hb]
    for ea, eb in zip(ha, hb):
        for x, y in zip(ea[:4], eb[:4]):
            assert abs(x - y) <= 2e-5 * max(1.0, abs(y)), (ea, eb)
    assert rel < 1e-5


def test_short_last_masked_batch_takes_the_masked_fallback(dev):
    from moleculesde_amd import hip, pretrain
    from moleculesde_amd.dataset import DatasetRunner, MoleculeStore, ResidentDataset
    args = pretrain.readme_args(emb_dim=64, SDE_coeff_generative_3Dto2D=0, batch_size=B, epochs=1)
    sizes = np.random.default_rng(9).integers(2, 25, size=27)
    store = MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=23))
    plan = store.epoch_plan(1, B, seed=2, mask_ratio=0.15, mask_seed=1)
    assert plan.n_batches == 4 and plan.n_full == 3
    tr = _trainer(args, dev, 5)
    rd = ResidentDataset(store, dev)
    runner = DatasetRunner(tr, rd, plan)
    p0 = tr.opt.flat_p.clone()
    assert runner.run(plan) == 4 and runner.fallbacks == 1
    torch.cuda.synchronize()
    assert int(rd.counter.cpu()) == 4 and int(rd.err.cpu()) == 0
    assert torch.isfinite(tr.opt.flat_p).all() and not torch.equal(tr.opt.flat_p, p0)
    with pytest.raises(ValueError, match="masking"):                 # the graph holds the masked gather: no unmasked epochs on it
        runner.run(store.epoch_plan(2, B, seed=2))
    hip.clear_row_bounds()


def _main_argv(tmp_path, monkeypatch):
    """A 20-molecule store file, the tiny masked configuration of pretrain.main, and every Trainer on the capturable noise
    source (the same draws whether a step is replayed or launched from the host)."""
    import moleculesde_amd.geom3d as G
    from moleculesde_amd import pretrain
    from moleculesde_amd.dataset import MoleculeStore
    sizes = np.random.default_rng(10).integers(2, 21, size=20)
    path = str(tmp_path / "store.pt")
    MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=24)).save(path)
    init = pretrain.Trainer.__init__

    def with_fixed_noise(self, args, device, noise=None, overlap_streams=True):
        init(self, args, device, noise=capturable_noise(G, device), overlap_streams=overlap_streams)
    monkeypatch.setattr(pretrain.Trainer, "__init__", with_fixed_noise)
    return ["--dataset_file", path, "--epochs", "1", "--batch_size", "8", "--emb_dim", "64", "--SDE_2Dto3D_model",
            "SDEModel2Dto3D_02", "--CL_similarity_metric", "EBM_node_dot_prod", "--SDE_coeff_generative_3Dto2D", "0",
            "--dropout_ratio", "0", "--SSL_masking_ratio", "0.15", "--mask_seed", "4"]


def test_pretrain_main_trains_on_masked_molecules(dev, tmp_path, capsys, monkeypatch):
    from moleculesde_amd import hip, pretrain
    out = pretrain.main(_main_argv(tmp_path, monkeypatch))
    printed = capsys.readouterr().out
    assert "epoch: 1" in printed and "SDE 2Dto3D Loss" in printed and "1 fell back" in printed
    assert len(out) == 1 and out[0][5] == math.ceil(20 / 8) and all(math.isfinite(v) for v in out[0][:4])
    hip.clear_row_bounds()


def test_pretrain_main_masked_replays_agree_with_eager(dev, tmp_path, monkeypatch):
    """pretrain.main --dataset_file ... --SSL_masking_ratio 0.15 through graph replays, then the same command with --eager on
    the same seeds: epoch losses within the tolerance of the eager-twin test above (2e-5 relative).  Under masking the --eager
    loop takes the captured runner's start (EagerDatasetRunner(start_plan=...): two warm-up updates on the first batch, draws
    seeded by the device step counter); without that the pair differs by those two updates and by its contrastive
    permutations (measured: CL loss 30.28 against 37.04), at any ratio."""
    from moleculesde_amd import hip, pretrain
    argv = _main_argv(tmp_path, monkeypatch)
    out = pretrain.main(argv)
    hip.clear_row_bounds()
    eager = pretrain.main(argv + ["--eager"])
    hip.clear_row_bounds()
    print("masked main, replays vs --eager:", out[0][:4], eager[0][:4])
    for x, y in zip(out[0][:4], eager[0][:4]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(y)), (out[0], eager[0])
