#!/usr/bin/env python3
"""Episodic few-shot evaluation driver with the reference's CLI / YAML surface
(test_phase/test_few_shot.py:36-134): 5-way `--shot`-shot, 15 queries per class, 2000 batches of
`ep_per_batch`=1 episode, seeds 12345, `acc +- 95 % CI` over per-batch accuracies.

MI355X-native differences (results are unchanged by them):
  * many batches are pushed through the HIP engine per launch (`--launch-batches`), because one
    80-100 image episode cannot fill the GPU; accuracies stay per batch, so the CI is the same;
  * multi-GPU = one process per GPU (torchrun), episodes sharded rank::world from the SAME sampler
    stream, one all-gather of the per-batch statistics at the end (parallel.py) instead of
    nn.DataParallel;
  * `--episodes` limits the number of batches (BASELINE config 1 uses 100) without changing the stream.

The protocol itself - seeds, launch loop, statistics exchange, averagers, result dict, command line - is `episodic.evaluate`, shared with
`eval_cached` and `eval_sauc`; this driver is its dense prototype-head route.

  python -m fewshot_vit_amd.test_few_shot --config few-shot-vit_amd/configs/test_synthetic.yaml --shot 5
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m fewshot_vit_amd.test_few_shot ...
"""
from . import episodic
from .episodic import build_model, default_launch_batches, fix_random_seeds      # noqa: F401  (the names this driver has always exported)


def evaluate(config, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False):
    """launch_batches: reference batches per engine launch; None (the default, also the CLI's) = `default_launch_batches` - the benched
    configuration (128 five-shot episodes of 100 images)."""
    out = episodic.evaluate(config, 5, episodic.proto_dense, episodic.reduce_batches, shot=shot, test_epochs=test_epochs, n_batch=n_batch,
                            ep_per_batch=ep_per_batch, launch_batches=launch_batches, numerics=numerics, rank=rank, world=world, device=device, log=log,
                            collect_pred=collect_pred)
    if out is not None:                                     # the reference driver's dict carries no image counters (eval_cached's does)
        del out['images_requested'], out['images_encoded']
    return out


def main():
    episodic.run_cli(evaluate, episodic.make_parser())


if __name__ == '__main__':
    main()
