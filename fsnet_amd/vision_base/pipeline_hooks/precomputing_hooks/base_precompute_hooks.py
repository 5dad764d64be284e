"""Hooks that run once before training (reference vision_base/pipeline_hooks/precomputing_hooks/
base_precompute_hooks.py): scripts/train.py builds cfg.precompute_hook, when the config has one, and calls it before
the training dataset is built."""


class BasePrecomputeHook(object):
    """Precomputing hooks take no call arguments; their constructor takes the parameters."""
    def __init__(self, *args, **kwargs):
        pass

    def __call__(self, *args, **kwargs):
        pass
