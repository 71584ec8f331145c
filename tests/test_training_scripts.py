"""What the training scripts write beside their checkpoints: config.json, the half of the checkpoint contract that benchmark_agent reads
(bird_view/utils/bz_utils.py).  Every script builds its config in build_config(parsed, rank, world, device), which needs no GPU; the files
under tests/fixtures/script_configs were written by the scripts as they stood before build_config existed, for the same two flag lines,
and the bytes are compared: the schema, the stringification and the scripts' known oddities (camera_args at top level in phase 0 and
under agent_args with a fixed offset in phase 1, num_workers, the stringified device) stay where a reader expects them."""
import importlib
import os

import pytest
import torch

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "script_configs")
LOG_DIR = "runs/pinned"
SHARED = ("--seed 7 --save_state --save_state_every 2 --resume --skip-nonfinite --clip-grad-norm 1 --accumulate 2 --lr-schedule cosine "
          "--warmup-steps 2 --lr-total-steps 10 --weight-decay 0.01 --ema-decay 0.9 --ema-eval --val-metrics --train-metrics "
          "--dataset_dir D --resident --resident-reserve-gb 2").split()
OWN = {"train_birdview": "--x_jitter 3 --y_jitter 2 --angle_jitter 4".split(), "train_image_phase0": ["--cache-teacher"],
       "train_image_phase1": ["--cache-teacher"]}


@pytest.mark.parametrize("flags", ["required", "options"])
@pytest.mark.parametrize("module", sorted(OWN))
def test_config_json_is_pinned(tmp_path, module, flags):
    from learningbycheating_amd.bird_view.utils.bz_utils import Experiment
    script = importlib.import_module("learningbycheating_amd.training." + module)
    argv = ["--log_dir", LOG_DIR] + (SHARED + OWN[module] if flags == "options" else [])
    with torch.random.fork_rng(devices=[]):               # (--seed seeds torch's generator where the config is built)
        config = script.build_config(script.parse_arguments(argv), 0, 1, torch.device("cuda", 0))
    assert config["rank"] == 0 and config["world_size"] == 1
    Experiment().init(str(tmp_path)).save_config({k: v for k, v in config.items() if k not in ("rank", "world_size")})      # (as train() saves it)
    with open(os.path.join(FIXTURES, "%s.%s.json" % (module, flags)), "rb") as f:
        want = f.read()
    assert (tmp_path / "config.json").read_bytes() == want
