"""World-2 data parallelism on CPU (gloo) with a compiled sed_eval(): the validation counts are all-reduced as int64, so
val_seg_f1 / val_seg_er / val_event_f1 are identical on both ranks and EQUAL the single-process values of the concatenated
validation shards (tests/sedeval_ref.py), and the merged counts are the exact sum."""
import os
import socket
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.45, 0.5)


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
    sed = M.sed_eval(THRESHOLDS, hop=S.output_hop(cfg))
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  ddp=S.wrap_ddp(model, device, world), metrics=[sed])
    g = torch.Generator().manual_seed(10 + rank)          # each rank its own shard, of its own size
    tb = [(torch.randn(2, 32, 64, 1, generator=g), (torch.rand(2, 2, 3, generator=g) > 0.5).float())]
    vb = [(torch.randn(4 + rank, 32, 64, 1, generator=g), (torch.rand(4 + rank, 2, 3, generator=g) > 0.5).float()) for _ in range(2)]
    hist = S.fit(model, Dataset.from_generator(lambda: iter(tb)).repeat(), epochs=1, steps_per_epoch=1,
                 validation_data=Dataset.from_generator(lambda: iter(vb)).repeat(), validation_steps=2, rank=rank, world=world,
                 verbose=False)
    own = sed.counter.counts()                                # this rank's shard: the all-reduce acted on a copy
    values = model._metrics.sed_values('val_', all_reduce=True)
    merged = sed.counter.state('cpu').clone()
    torch.distributed.all_reduce(merged)
    model.eval()
    with torch.no_grad():
        yp = torch.cat([model(x) for x, _ in vb])
    torch.save({"row": hist[0], "values": values, "own": own, "merged": merged, "yt": torch.cat([y for _, y in vb]), "yp": yp},
               os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


def test_sed_values_all_reduced_over_two_ranks(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sedeval_ref as R
    from challenge_amd import metrics as M
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    yt = np.concatenate([x["yt"].numpy() for x in res])
    yp = np.concatenate([x["yp"].numpy() for x in res])
    want = R.counts(yt, yp, THRESHOLDS, hop=8192)
    single = M.MetricSet([M.sed_eval(THRESHOLDS, hop=8192)])            # one process, the concatenated batches
    single(torch.from_numpy(yt), torch.from_numpy(yp), 'val')
    values = single.sed_values('val_')

    def same(a, b):
        return a == b or (a != a and b != b)
    for x in res:
        for key in ('val_seg_f1', 'val_seg_er', 'val_event_f1'):
            assert same(x["row"][key], values[key]) and same(x["values"][key], values[key]), (key, x["row"], values)
        assert x["row"]['val_loss'] == res[0]["row"]['val_loss']
        assert torch.equal(x["merged"], res[0]["own"] + res[1]["own"])
    assert not torch.equal(res[0]["own"], res[1]["own"])
    assert np.array_equal(res[0]["merged"].numpy(), want) and int(want[0, 3, 3]) == 8 + 10
