"""World-2 data parallelism on CPU (gloo) with compiled metrics: the epoch metrics are all-reduced as sums and counts, so
val_er is identical on both ranks and equals the mean over the ranks' own validation clips."""
import os
import socket
import sys

import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    model.compile(S.make_optimizer(cfg, model.parameters()), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  ddp=S.wrap_ddp(model, device, world), metrics=[M.cos_sim, M.f1_score(), M.er_score(smoothing=False)])
    g = torch.Generator().manual_seed(10 + rank)          # each rank its own shard
    tb = [(torch.randn(2, 32, 64, 1, generator=g), (torch.rand(2, 2, 3, generator=g) > 0.5).float())]
    vb = [(torch.randn(3, 32, 64, 1, generator=g), (torch.rand(3, 2, 3, generator=g) > 0.5).float()) for _ in range(2)]
    hist = S.fit(model, Dataset.from_generator(lambda: iter(tb)).repeat(), epochs=1, steps_per_epoch=1,
                 validation_data=Dataset.from_generator(lambda: iter(vb)).repeat(), validation_steps=2, rank=rank, world=world,
                 verbose=False)
    model.eval()
    with torch.no_grad():
        own = torch.cat([M.er_host(y, model(x)) for x, y in vb]).double().mean()
    torch.save({"row": hist[0], "own": float(own)}, os.path.join(out_dir, f"rank{rank}.pt"))
    torch.distributed.destroy_process_group()


def test_val_er_all_reduced_over_two_ranks(tmp_path):
    world = 2
    mp.start_processes(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True, start_method="spawn")
    res = [torch.load(os.path.join(tmp_path, f"rank{r}.pt")) for r in range(world)]
    rows = [x["row"] for x in res]
    for key in ('er', 'val_er', 'f1_score', 'val_f1_score', 'cos_sim', 'val_cos_sim'):
        assert rows[0][key] == rows[1][key], key
    mean = sum(x["own"] for x in res) / world
    assert abs(rows[0]['val_er'] - mean) <= 1e-12, (rows[0]['val_er'], mean)
