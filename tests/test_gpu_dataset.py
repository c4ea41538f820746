"""Pretraining on a device-resident molecule store (moleculesde_amd/dataset.py, csrc/dataset.hip).

1. The gathered raw blob equals bucket.pack_raw of the same molecules, collated on the host with centred_positions, word for
   word -- coordinates and zeroed tails included.
2. {gather + device-side plans} captured in one graph: replay k builds batch k, the counter reads k + 1.
3. The gather's guards: an invalid batch writes nothing and raises the gather's own error word; the host API refuses the
   same inputs before any launch.
4. DatasetRunner trains like StreamRunner fed with the same batches collated on the host.
5. The short last batch takes the exact-size fallback.  6. pretrain.main --dataset_file.
"""
import math
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dataset_cases import capturable_noise, off_centre_molecules  # noqa: E402
from helpers import disable_dropout  # noqa: E402

B = 8
SIZES = [1, 2, 17, 31, 32, 32, 1, 2] + [3, 24, 9, 14, 20, 6, 11, 5, 13, 16, 8, 12, 19, 7, 15, 10, 18, 4, 22, 21, 25, 30, 23, 28, 3, 9,
                                        14, 12, 6, 27, 26, 29]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    from moleculesde_amd import _lib
    _lib.load()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _collect_graphs_and_buckets_here():
    """Buckets (bucket <-> batch) and the trainers that hold captured graphs are cyclic garbage: collect them when this module
    is done, with the device idle, instead of whenever the collector next runs inside some later test (moleculesde_amd/slabs.py,
    no_gc: destroying a graph or releasing pool memory at an arbitrary moment is a hazard of its own)."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def case(dev):
    """The store of 40 off-centre molecules (sizes 1, 2, 17, 31, 32 among them), its first epoch plan, the capacities of
    caps_for and, per batch, the host batch and the blob pack_raw makes of it (computed once, never modified)."""
    from moleculesde_amd import bucket as BK
    from moleculesde_amd.dataset import MoleculeStore, ResidentDataset, caps_for
    assert len(SIZES) == 40
    store = MoleculeStore.from_molecules(off_centre_molecules(SIZES, seed=21))
    plan = store.epoch_plan(1, B, seed=3)
    caps = caps_for(plan)
    assert plan.n_batches == plan.n_full == 5 and caps.n_max == 32
    host = [store.collate(plan.molecules(k)) for k in range(5)]
    c = types.SimpleNamespace(store=store, plan=plan, caps=caps, host=host, BK=BK,
                              blobs=[BK.pack_raw(b, caps) for b in host], rd=ResidentDataset(store, dev))
    c.atoms = [plan.need(k)["N"] for k in range(5)]
    return c


def test_gathered_blob_equals_pack_raw_word_for_word(dev, case):
    c, BK = case, case.BK
    bk = BK.Bucket(c.caps, dev)
    c.rd.begin_epoch(c.plan)
    ks = sorted({0, 2, c.plan.n_full - 1}, key=lambda k: -c.atoms[k])
    ks = [ks[0], ks[-1]] + ks[1:-1]              # the most atoms first, the fewest second: stale tails would show
    assert c.atoms[ks[0]] > c.atoms[ks[1]]
    for k in ks:
        c.rd.gather(bk, c.plan, k)
        got = bk.raw.cpu()
        diff = (got != c.blobs[k]).nonzero().flatten()
        assert diff.numel() == 0, (k, diff[:8].tolist(), {n: o for n, o in bk.layout.items()})
        assert int(c.rd.counter.cpu()) == k + 1 and int(c.rd.err.cpu()) == 0
    # remove_center=0: the coordinates are the store's own
    k = ks[0]
    c.rd.gather(bk, c.plan, k, remove_center=False)
    want = BK.pack_raw(c.store.collate(c.plan.molecules(k), remove_center=False), c.caps)
    assert torch.equal(bk.raw.cpu(), want) and not torch.equal(want, c.blobs[k])


def test_captured_gather_and_plan_follow_the_device_counter(dev, case):
    from moleculesde_amd import plan as P
    c, BK = case, case.BK
    bk = BK.Bucket(c.caps, dev)
    rd = c.rd
    rd.begin_epoch(c.plan)
    body = lambda: (rd.launch_gather(bk.raw, bk.layout, c.caps), bk.build_plan_on_device())
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()                                   # eager warm-up call
    torch.cuda.synchronize()
    rd.counter.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        body()
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bk.raw.cpu(), c.blobs[k]), k
        assert int(rd.counter.cpu()) == k + 1 and int(rd.err.cpu()) == 0
        ok, sizes = bk.check()
        assert ok, sizes
        hp = P.build_plan(c.host[k].clone())
        N, pl = hp.N, bk.plan
        assert sizes["N"] == N and sizes["E_b"] == hp.bond.E and sizes["E_e"] == hp.ext.E
        assert torch.equal(pl.mol_ptr.cpu(), hp.mol_ptr.cpu())
        assert torch.equal(pl.bond.rowptr[:N + 1].cpu(), hp.bond.rowptr.cpu())
        assert torch.equal(pl.ext.rowptr[:N + 1].cpu(), hp.ext.rowptr.cpu())


def test_guards_write_nothing_and_set_the_error_word(dev, case):
    c, BK = case, case.BK
    rd, plan, M = c.rd, c.plan, len(c.store)
    rd.begin_epoch(plan)
    k_big = int(np.argmax(c.atoms))
    k32 = next(k for k in range(5) if plan.need(k)["n_max"] == 32)
    tight = types.SimpleNamespace(B=B, N=c.atoms[k_big] - 1, E_b=c.caps.E_b, n_max=32)      # one atom row too few
    bad_perm = torch.from_numpy(plan.perm.astype(np.int32)).to(dev)
    bad_perm[3] = M
    GUARD, SENT = 64, -0x5A5A5A5B
    cases = [("perm entry == M", c.caps, dict(perm=bad_perm), 0, 1),
             ("32 atoms, n_max 24", c.caps, dict(n_max=24), k32, 2),
             ("capacity one row short", tight, dict(), k_big, 4),
             ("fewer than B remain", c.caps, dict(n_avail=B * 5 - 1), 4, 8)]
    for what, caps, kw, k, bit in cases:
        lay = BK.raw_layout(caps)
        buf = torch.full((GUARD + lay["_total"] + GUARD,), SENT, dtype=torch.int32, device=dev)
        blob = buf[GUARD:GUARD + lay["_total"]]
        ctr = torch.zeros(1, dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        # a valid previous batch (the smallest one: it fits every capacity used here)
        k_prev = int(np.argmin(c.atoms))
        ctr.fill_(k_prev)
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err)
        before = buf.clone()
        assert int(err.cpu()) == 0 and bool((before[GUARD:-GUARD] != SENT).any())
        ctr.fill_(k)
        rd.launch_gather(blob, lay, caps, counter=ctr, err=err, **kw)
        torch.cuda.synchronize()
        assert int(err.cpu()) == bit, (what, int(err.cpu()))
        assert torch.equal(buf, before), what + ": the blob (and its guard bands) must be untouched"
        assert bool((buf[:GUARD] == SENT).all()) and bool((buf[-GUARD:] == SENT).all()), what
        assert int(ctr.cpu()) == k + 1
    # the host API refuses the same inputs before any launch
    with pytest.raises(ValueError, match="outside"):
        c.store.epoch_plan(1, B, perm=bad_perm.cpu())
    caps24 = BK.Caps.covering([plan.need(k) for k in range(5)], n_max=24)
    small = BK.Caps.covering([plan.need(int(np.argmin(c.atoms)))])
    assert not plan.fits(caps24)[k32] and not plan.fits(small)[k_big]
    for caps, k in ((caps24, k32), (small, k_big)):
        bk = BK.Bucket(caps, dev)
        before = bk.raw.clone()
        with pytest.raises(BK.BucketOverflow):
            rd.gather(bk, plan, k)
        assert torch.equal(bk.raw, before)
    assert int(rd.err.cpu()) == 0


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


def test_dataset_runner_matches_stream_runner_on_the_same_batches(dev):
    """Run A: DatasetRunner through train_epochs.  Run B: StreamRunner(n_max=24) on the same batches collated on the host in
    the same epoch order with centred_positions, same capacities, same warm-up batch.  Tolerances: those of
    test_stream_runner_matches_its_eager_twin_and_main_runs (replay against its eager twin); the runs are in fact bitwise
    equal (same blob words, same kernels in the same order), and that is asserted last."""
    from moleculesde_amd import bucket as BK, hip, pretrain
    from moleculesde_amd.dataset import DatasetRunner, MoleculeStore, ResidentDataset
    args = pretrain.readme_args(emb_dim=64, SDE_coeff_generative_3Dto2D=0, batch_size=B, epochs=2)
    args.output_model_dir = ""
    sizes = np.random.default_rng(8).integers(2, 25, size=24)
    store = MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=22))
    plans = {e: store.epoch_plan(e, B, seed=1) for e in (1, 2)}
    host = {e: [store.collate(plans[e].molecules(k)) for k in range(3)] for e in (1, 2)}
    caps = BK.Caps.covering([BK.raw_sizes(b) for e in (1, 2) for b in host[e]], n_max=24)
    quiet = lambda *_: None
    # A
    tr = _trainer(args, dev, 11)
    ra = DatasetRunner(tr, ResidentDataset(store, dev), plans[1], caps=caps)
    ha = pretrain.train_epochs(args, tr, ra, lambda e: (plans[e], None), out=quiet)
    torch.cuda.synchronize()
    pa = tr.opt.flat_p.clone()
    assert ra.fallbacks == 0 and int(ra.rd.counter.cpu()) == 3 and int(ra.rd.err.cpu()) == 0
    hip.clear_row_bounds()
    # B
    tr = _trainer(args, dev, 11)
    rb = pretrain.StreamRunner(tr, host[1] + host[2], n_max=24)
    assert rb.caps.as_dict() == caps.as_dict()
    blobs = {e: [rb.pack(b) for b in host[e]] for e in (1, 2)}
    hb = pretrain.train_epochs(args, tr, rb, lambda e: (blobs[e], 3), out=quiet)
    torch.cuda.synchronize()
    pb = tr.opt.flat_p.clone()
    hip.clear_row_bounds()
    rel = float((pa - pb).norm() / pb.norm())
    print("dataset runner vs stream runner:", [e[:4] for e in ha], [e[:4] for e in hb], "params rel", rel,
          "bitwise", torch.equal(pa, pb))
    assert [e[5] for e in ha] == [3, 3] == [e[5] for e in hb]
    for ea, eb in zip(ha, hb):
        for x, y in zip(ea[:4], eb[:4]):
            assert abs(x - y) <= 2e-5 * max(1.0, abs(y)), (ea, eb)
    assert rel < 1e-5
    # the two feeds put the same words into the same graph's inputs: measured bitwise equal on the MI355X, so that is asserted
    assert [e[:4] for e in ha] == [e[:4] for e in hb] and torch.equal(pa, pb)


def test_short_last_batch_takes_the_fallback_and_runner_refuses_small_caps(dev):
    from moleculesde_amd import bucket as BK, hip, pretrain
    from moleculesde_amd.dataset import DatasetRunner, MoleculeStore, ResidentDataset
    args = pretrain.readme_args(emb_dim=64, SDE_coeff_generative_3Dto2D=0, batch_size=B, epochs=1)
    sizes = np.random.default_rng(9).integers(2, 25, size=27)
    store = MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=23))
    plan = store.epoch_plan(1, B, seed=2)
    assert plan.n_batches == 4 and plan.n_full == 3
    tr = _trainer(args, dev, 5)
    rd = ResidentDataset(store, dev)
    nd = plan.need(0)
    assert nd["N"] > 64
    with pytest.raises(BK.BucketOverflow):       # too few atom rows for the first batch: refused before any launch
        DatasetRunner(tr, rd, plan, caps=BK.Caps(B, 64, nd["E_b"], nd["E_e"], nd["E_r"], nd["P"], 24))
    runner = DatasetRunner(tr, rd, plan)
    p0 = tr.opt.flat_p.clone()
    assert runner.run(plan) == 4 and runner.fallbacks == 1
    torch.cuda.synchronize()
    assert int(rd.counter.cpu()) == 4 and int(rd.err.cpu()) == 0
    assert torch.isfinite(tr.opt.flat_p).all() and not torch.equal(tr.opt.flat_p, p0)
    hip.clear_row_bounds()


def test_pretrain_main_trains_on_a_dataset_file(dev, tmp_path, capsys):
    from moleculesde_amd import hip, pretrain
    from moleculesde_amd.dataset import MoleculeStore
    sizes = np.random.default_rng(10).integers(2, 21, size=20)
    path = str(tmp_path / "store.pt")
    MoleculeStore.from_molecules(off_centre_molecules(sizes, seed=24)).save(path)
    out = pretrain.main(["--dataset_file", path, "--epochs", "1", "--batch_size", "8", "--emb_dim", "64", "--SDE_2Dto3D_model",
                         "SDEModel2Dto3D_02", "--CL_similarity_metric", "EBM_node_dot_prod", "--SDE_coeff_generative_3Dto2D", "0",
                         "--dropout_ratio", "0"])
    printed = capsys.readouterr().out
    assert "epoch: 1" in printed and "SDE 2Dto3D Loss" in printed and "1 fell back" in printed
    assert len(out) == 1 and out[0][5] == math.ceil(20 / 8)
    assert all(math.isfinite(v) for v in out[0][:4])
    hip.clear_row_bounds()
