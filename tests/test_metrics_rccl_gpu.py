"""The metric launch inside the graphed training step under DistributedDataParallel over RCCL: a world-size-1 'nccl'
process group (IRIS_FORCE_PG=1) in a fresh process, so GraphedTrainStep takes its capture path with the bucketed gradient
all-reduce in the graph.  The captured metrics must equal the standalone callables on the step's predictions, leave the
training bitwise where the same step without metrics leaves it, and `fit` must log them through its collectives."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      IRIS_FORCE_PG="1")
    import torch.distributed as dist
    from challenge_amd import metrics as M
    from challenge_amd import sj_train as S
    S.configure_miopen()
    rank, world, device = S.init_distributed()
    assert dist.is_initialized() and dist.get_backend() == "nccl" and world == 1
    cfg = S.ARGS().get(['--v', '9', '--n_mels', '32', '--n_frame', '64', '--n_chan', '1', '--batch_size', '8'])
    g = torch.Generator().manual_seed(7)
    x = torch.randn(8, 32, 64, 1, generator=g).to(device).contiguous(memory_format=torch.channels_last)
    y = (torch.rand(8, 2, 3, generator=g) > 0.6).float().to(device)

    def fresh(metrics):
        torch.manual_seed(0)
        m = S.get_model(cfg).to(device).to(memory_format=torch.channels_last)
        m.compile(S.make_optimizer(cfg, m.parameters(), capturable=True), S.binary_crossentropy, clipvalue=cfg.clipvalue,
                  ddp=S.wrap_ddp(m, device, world), metrics=metrics)
        return m
    plain = fresh(None)
    f1 = M.f1_score()
    with_m = fresh([M.cos_sim, f1, M.er_score(smoothing=False)])
    s0 = S.GraphedTrainStep(plain, (x, y), preserve_state=True)
    s1 = S.GraphedTrainStep(with_m, (x, y), preserve_state=True)
    assert s0.world == 1 and s1.world == 1        # the capture holds the RCCL all-reduce
    assert float(f1.states[device].abs().sum()) == 0.0
    ref_f1 = M.f1_score()
    for _ in range(3):
        s0((x, y))
        out = s1((x, y))
        torch.cuda.synchronize(device)
        yp = s1.y_pred
        assert torch.equal(out['er'], M.er_score(smoothing=False)(y, yp))
        assert torch.equal(out['cos_sim'], M.event_metrics(y, yp, want_cos=True)['cos_sim'])
        assert torch.equal(out['f1_score'], ref_f1(y, yp))
    same = all(torch.equal(a, b) for a, b in zip(plain.parameters(), with_m.parameters()))
    # fit through the RCCL collectives: graph by default, rows with the metrics and their val_ twins
    fm = fresh([M.cos_sim, M.f1_score(), M.er_score(smoothing=False)])

    def forever():
        while True:
            yield x, y
    hist = S.fit(fm, forever(), epochs=1, steps_per_epoch=3, validation_data=forever(), validation_steps=2, rank=0, world=1,
                 verbose=False)
    torch.save({"same": same, "row": hist[0]}, os.path.join(out_dir, "res.pt"))
    dist.destroy_process_group()


def test_metrics_in_the_graphed_step_under_rccl_world1(tmp_path):
    assert torch.cuda.is_available()
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    res = torch.load(tmp_path / "res.pt")
    assert res["same"]
    for key in ('er', 'val_er', 'f1_score', 'val_f1_score', 'cos_sim', 'val_cos_sim'):
        assert key in res["row"] and res["row"][key] == res["row"][key], (key, res["row"])
