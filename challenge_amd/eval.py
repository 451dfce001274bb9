"""Drop-in counterpart of the reference's eval.py: score a trained model against sample_answer.json.

    python -m challenge_amd.eval --name <run name> [--p] [--path DIR] [--verbose True] [--curves OUT.json [--curve_bins 1024]]
                                [--sed_eval OUT.json [--sed_thresholds 0.5]] [--psds OUT.json [--psds_scenario 1,2]]

loads <path>/<name>.pt (this package's checkpoint) - or, for a model trained with the reference, its Keras weights as
<path>/<name>.npz (scripts/dump_keras_weights.py) - and runs metrics.evaluate on the *.wav files of the working directory.
`--curves OUT.json` also writes the threshold-free numbers of the files' frame posteriors against the answer's frame labels
(metrics.ScoreHistogram.compute: ROC-AUC, average precision, best F1 and its threshold, calibration error per class, with the
macro values) as JSON.
`--sed_eval OUT.json` writes the segment- and event-based measures of sed_eval / DCASE (metrics.SedEval.compute: 1 s segments;
200 ms onset collar, offset collar max(200 ms, 50 % of the event); greedy matching per class) of the same posteriors and labels
at every threshold of `--sed_thresholds`, a comma list (default 0.5).
`--psds OUT.json` writes the polyphonic sound detection score (metrics.Psds.compute: intersection criteria, 50 thresholds) of the
same posteriors and labels under every scenario of `--psds_scenario`, a comma list of 1 and 2 (default both), as {scenario: result}.
`--p` parses model / v / n_mels / n_chan / n_frame out of the run name as eval.py:51-62 does."""
from __future__ import annotations

import json
import os

import numpy as np
import torch

from .data_utils import minmax_log_on_mel  # noqa: F401  (eval.py:13-27: the same batch-wise min-max + log)
from .metrics import Challenge_Metric, evaluate, get_er, output_to_metric  # noqa: F401


def second2frame(seconds: list, frame_num, resolution):
    """eval.py:30-38: [[class, start s, end s], ...] -> frame labels [frame_num, 3] (overlaps add up)."""
    frames = np.zeros([frame_num, 3], dtype=np.float32)
    for second in seconds:
        class_num = second[0]
        start = int(np.round(second[1] * resolution))
        end = int(np.round(second[2] * resolution))
        frames[start:end, class_num] += 1
    return torch.from_numpy(frames)


def parse_name(config):
    """eval.py:51-62: the run name's fields -> model_type / model / v / n_mels / n_chan / n_frame.  The reference drops one
    leading token in front of the model field; here every one is dropped, so a --name with an underscore of its own
    ('pcen_learn', 'filter_pcen') round-trips through `fit.run_name` too (such names raised before; names with one leading
    token or none parse as they did).  As in the reference, a --name token that itself starts with 'B' or 'v' is taken for the
    model field: keep such tokens out of --name."""
    parsed = config.name.split('_')
    while len(parsed) > 1 and parsed[0][:1] not in ('B', 'v'):
        parsed = parsed[1:]
    if parsed[0] == 'vad':
        config.model_type = 'vad'
        config.model = 1
    else:
        config.model = int(parsed[0][-1])
    config.v = int(parsed[1][-1])
    config.n_mels = int(parsed[6][3:])
    config.n_chan = int(parsed[7][-1])
    config.n_frame = int(parsed[9].split('framelen')[-1])
    return config


def load_model(config, path: str = '', device=None):
    from .model import get_model, load_keras_weights
    if device is None:
        device = torch.device('cuda', 0) if torch.cuda.is_available() else torch.device('cpu')
    model = get_model(config).to(device)
    if device.type == 'cuda':
        model = model.to(memory_format=torch.channels_last)
    base = os.path.join(path, config.name)
    if base.endswith('.h5'):
        base = base[:-3]
    if os.path.exists(base + '.pt'):
        model.load_state_dict(torch.load(base + '.pt', map_location=device))
    elif os.path.exists(base + '.npz'):
        load_keras_weights(model, base + '.npz')
    else:
        raise FileNotFoundError(f"neither {base}.pt nor {base}.npz")
    model.eval()
    return model


class _PsdsFanOut:
    """One criteria set per launch: two scenarios are two Psds objects, fed the same tensors; `compute` is {scenario: result}."""

    def __init__(self, scenarios):
        from .metrics import Psds
        self.scored = {sc: Psds(3, sc) for sc in scenarios}

    def update(self, y_true, y_pred):
        for p in self.scored.values():
            p.update(y_true, y_pred)

    def compute(self):
        return {str(sc): p.compute() for sc, p in self.scored.items()}


def build_args():
    """The trainer's flags (the model is described by them) plus this tool's own."""
    from .sj_train import ARGS
    config = ARGS(trainer_flags=False)
    config.args.add_argument('--verbose', help='verbose', type=bool, default=True)
    config.args.add_argument('--p', help='parsing name', action='store_true')
    config.args.add_argument('--path', type=str, default='')
    config.args.add_argument('--curves', type=str, default=None, metavar='OUT.json',
                             help='also write ROC-AUC / average precision / best F1 per class and their macro values, from the score '
                                  'histogram of the frame posteriors, to this file')
    config.args.add_argument('--curve_bins', type=int, default=1024)
    from .sj_train import _sed_thresholds
    config.args.add_argument('--sed_eval', type=str, default=None, metavar='OUT.json',
                             help='also write segment-based F1 / ER and event-based F1 / ER (metrics.SedEval) of the frame posteriors '
                                  'at every threshold of --sed_thresholds to this file')
    config.args.add_argument('--sed_thresholds', type=_sed_thresholds, default=(0.5,), metavar='THRESHOLDS',
                             help='comma list of up to 16 increasing thresholds for --sed_eval (default 0.5)')
    config.args.add_argument('--psds', type=str, default=None, metavar='OUT.json',
                             help='also write the polyphonic sound detection score (metrics.Psds) of the frame posteriors under every '
                                  'scenario of --psds_scenario to this file')
    config.args.add_argument('--psds_scenario', type=_psds_scenarios, default=(1, 2), metavar='SCENARIOS',
                             help='comma list of DCASE scenarios (1, 2) for --psds (default 1,2)')
    return config


def _psds_scenarios(text):
    import argparse
    try:
        out = tuple(int(v) for v in text.split(','))
    except ValueError:
        out = ()
    if not out or any(v not in (1, 2) for v in out) or len(set(out)) != len(out):
        raise argparse.ArgumentTypeError(f"--psds_scenario: a comma list of distinct scenarios out of 1, 2, got {text!r}")
    return out


def main(argv=None):
    config = build_args().get(argv)
    if config.p:
        parse_name(config)
    model = load_model(config, config.path)
    from .metrics import ScoreHistogram, SedEval
    asked = {}   # `evaluate`'s keyword -> (the file to write, the counter whose compute() it holds)
    if config.curves:
        asked['curves'] = (config.curves, ScoreHistogram(3, config.curve_bins))
    if config.sed_eval:
        asked['sed'] = (config.sed_eval, SedEval(3, config.sed_thresholds or (0.5,)))
    if config.psds:
        asked['psds'] = (config.psds, _PsdsFanOut(config.psds_scenario))
    scores = evaluate(config, model, verbose=config.verbose, **{key: counter for key, (_, counter) in asked.items()})
    for path, counter in asked.values():
        with open(path, 'w') as f:
            json.dump(counter.compute(), f, indent=1)
    return scores


if __name__ == "__main__":
    main()
