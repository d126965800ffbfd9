#!/usr/bin/env python3
"""The reference's `test_few_shot.py --sauc` (test_phase/, meta_tuning_sun_m/test_few_shot.py:42-45,95-112, sun_meta_training/): 2-way episodes, the
queries scored against the single prototype of class 0 (`x_shot[:, 0]`) and reduced by ROC-AUC instead of soft-max.  Same CLI / YAML surface, episode
stream, seeds and launch batching as `test_few_shot.evaluate` - all of them run `episodic.evaluate` -; with `sauc` on, every launch is two encoder
passes and one `ops.proto_auc` call - no per-episode host sync - and the multi-rank path exchanges the AUCs through the same
`parallel.gather_in_stream_order` call.

`--feature-cache` / `feature_cache=True` (off by default): a launch encodes only the images no earlier launch has seen into a
`feature_table.FeatureTable` and reduces over its rows (`FeatureTable.auc`, fsvit_proto_auc_gather) - the same `va_lst` from at most one encoder pass
per image of the split.  Without `--sauc` the switch is `eval_cached.evaluate`'s.

  python -m fewshot_vit_amd.eval_sauc --config few-shot-vit_amd/configs/test_synthetic.yaml --shot 1 --sauc [--feature-cache]"""
from . import episodic, eval_cached


def evaluate(config, shot=1, test_epochs=1, n_batch=2000, ep_per_batch=1, launch_batches=None, numerics=None,
             rank=0, world=1, device=None, log=print, collect_pred=False, sauc=False, feature_cache=False):
    """sauc=False: `eval_cached.evaluate` - `test_few_shot.evaluate` itself with the cache off, plus the two image counters.  sauc=True: the same dict,
    where `va_lst` holds one AUC per EPISODE as the reference's loop appends them (:107-112), `acc` their mean, `ci` their 95 % interval and `loss` the
    untouched averager's value; out['images_requested'] / out['images_encoded'] are the images this rank's launches read / pushed through the encoder
    (equal without the cache)."""
    kw = dict(shot=shot, test_epochs=test_epochs, n_batch=n_batch, ep_per_batch=ep_per_batch, launch_batches=launch_batches, numerics=numerics,
              rank=rank, world=world, device=device, log=log)
    if not sauc:                                            # (both drivers carry the same keys, whatever the switches)
        return eval_cached.evaluate(config, collect_pred=collect_pred, feature_cache=feature_cache, **kw)
    if collect_pred:
        raise ValueError('collect_pred: --sauc scores against one prototype, there is no per-query arg-max to collect')
    return episodic.evaluate(config, 2, episodic.auc_table if feature_cache else episodic.auc_dense, episodic.reduce_episodes, **kw)      # 2-way (:42-46)


def make_parser():
    return episodic.make_parser(sauc=True, feature_cache=True, prog='python -m fewshot_vit_amd.eval_sauc')


def main(argv=None):
    episodic.run_cli(evaluate, make_parser(), argv)


if __name__ == '__main__':
    main()
