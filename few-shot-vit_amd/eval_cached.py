#!/usr/bin/env python3
"""Episodic few-shot evaluation from a feature table: `test_few_shot`'s CLI and `evaluate()` with one more switch, `--feature-cache` /
`feature_cache=True` (off by default: then this is `test_few_shot.evaluate`'s dense route, plus the two image counters).

Both settings run `episodic.evaluate` - one sampler, one launch loop, one statistics exchange.  With the switch on, a launch
encodes only the images no earlier launch has seen, into a `feature_table.FeatureTable`, and the episode head reads its rows through the sampler's
index table (fsvit_proto_head_gather): the same `va_lst`, accuracy, CI and loss from 12 000 encoder passes instead of the 160 000 (1-shot) / 200 000
(5-shot) of the reference's 2000-episode protocol.  Multi-GPU: every rank keeps its own table and encodes what its own batches touch (an image two
ranks draw is encoded on both); the sharding and the one exchange stay as they are.

  python -m fewshot_vit_amd.eval_cached --config few-shot-vit_amd/configs/test_synthetic.yaml --shot 5 --feature-cache
"""
from . import episodic


def evaluate(config, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False, feature_cache=False):
    """The arguments and the result dict of `test_few_shot.evaluate`, plus out['images_requested'] / out['images_encoded']: the images this rank's batches
    named / pushed through the encoder (equal without the cache)."""
    return episodic.evaluate(config, 5, episodic.proto_table if feature_cache else episodic.proto_dense, episodic.reduce_batches, shot=shot,
                             test_epochs=test_epochs, n_batch=n_batch, ep_per_batch=ep_per_batch, launch_batches=launch_batches, numerics=numerics,
                             rank=rank, world=world, device=device, log=log, collect_pred=collect_pred)


def main(argv=None):
    episodic.run_cli(evaluate, episodic.make_parser(feature_cache=True, description=__doc__.split('\n')[0]), argv)


if __name__ == '__main__':
    main()
