"""World-2 data parallelism on CPU (gloo) with a compiled psds(): the validation counts are all-reduced as int64, so val_psds is
identical on both ranks and EQUALS the single-process value of the concatenated validation shards (tests/psds_ref.py), and the
merged counts are the exact sum."""
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO = 2


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    from challenge_amd import metrics as M
    from challenge_amd import sj_train as S
    from challenge_amd.dataset import Dataset
    r, w, device = S.init_distributed()
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1'])
    torch.manual_seed(0)
    model = S.get_model(cfg)
    score = M.psds(SCENARIO, hop=S.output_hop(cfg))
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  ddp=S.wrap_ddp(model, device, world), metrics=[score])
    g = torch.Generator().manual_seed(10 + rank)          # each rank its own shard, of its own size
    tb = [(torch.randn(2, 32, 64, 1, generator=g), (torch.rand(2, 2, 3, generator=g) > 0.5).float())]
    vb = [(torch.randn(4 + rank, 32, 64, 1, generator=g), (torch.rand(4 + rank, 2, 3, generator=g) > 0.5).float()) for _ in range(2)]
    hist = S.fit(model, Dataset.from_generator(lambda: iter(tb)).repeat(), epochs=1, steps_per_epoch=1,
                 validation_data=Dataset.from_generator(lambda: iter(vb)).repeat(), validation_steps=2, rank=rank, world=world,
                 verbose=False)
    own = score.counter.counts()                             # this rank's shard: the all-reduce acted on a copy
    values = model._metrics.psds_values('val_', all_reduce=True)
    merged = score.counter.state('cpu').clone()
    torch.distributed.all_reduce(merged)
    model.eval()
    with torch.no_grad():
        yp = torch.cat([model(x) for x, _ in vb])
    torch.save({"row": hist[0], "values": values, "own": own, "merged": merged, "yt": torch.cat([y for _, y in vb]), "yp": yp},
               os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


def test_psds_values_all_reduced_over_two_ranks(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import psds_ref as R
    from challenge_amd import metrics as M
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    yt = np.concatenate([x["yt"].numpy() for x in res])
    yp = np.concatenate([x["yp"].numpy() for x in res])
    want = R.counts(yt, yp, M.psds_default_thresholds(), dtc_pct=10, gtc_pct=10, cttc_pct=30)
    single = M.MetricSet([M.psds(SCENARIO, hop=8192)])                   # one process, the concatenated batches
    single(torch.from_numpy(yt), torch.from_numpy(yp), 'val')
    value = single.psds_values('val_')['val_psds']
    assert value == value and value == M.psds_metrics(want, M.psds_default_thresholds(), 8192, 16000, 0.5, 1.0)['psds']
    for x in res:
        assert x["row"]['val_psds'] == value and x["values"] == {'val_psds': value}, (x["row"], x["values"], value)
        assert x["row"]['val_loss'] == res[0]["row"]['val_loss']
        assert torch.equal(x["merged"], res[0]["own"] + res[1]["own"])
    assert not torch.equal(res[0]["own"], res[1]["own"])
    assert np.array_equal(res[0]["merged"].numpy(), want) and int(want[50, 0, 3]) == 2 * (8 + 10)
