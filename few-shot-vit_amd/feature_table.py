"""FeatureTable: every image of a dataset goes through the encoder once, the episodes read their rows through the sampler's index table.

The reference's evaluation (test_phase/test_few_shot.py:76-92) encodes every image an episode draws: 2000 five-way episodes over a 12 000-image
test split are 160 000 (1-shot) or 200 000 (5-shot) encoder passes.  In eval mode the transform is deterministic (Resize -> CenterCrop), BatchNorm
uses its running statistics and the engines give the same bits for an image whatever launch it sits in, so the feature of image i is a function
of i alone.  The table keeps it: `ensure` encodes the images it has not seen (ascending image order, the engine's chunks) and hands back slot numbers,
`episodes` runs the episode head over those slots in one launch (fsvit_proto_head_gather, head.hip) - no image tensor, no feature copy.

The bookkeeping (`slot_of`, the counters, the order of the encoder calls) is host-side numpy and does not look at the device; only `episodes` and
`for_dataset` need the GPU.  The table does not watch the weights: call `reset()` when they change."""
import numpy as np
import torch


class FeatureTable:

    def __init__(self, encode_fn, n_images, dim, device, chunk_images=None):
        """encode_fn(index) -> [len(index), dim] features on `device` for a sorted 1-d int64 host tensor of image indices; it is handed at most
        `chunk_images` indices per call (None: no limit)."""
        if int(n_images) < 1 or int(dim) < 1:
            raise ValueError('FeatureTable needs n_images >= 1 and dim >= 1')
        if chunk_images is not None and int(chunk_images) < 1:
            raise ValueError('chunk_images >= 1')
        self.encode_fn = encode_fn
        self.n_images, self.dim = int(n_images), int(dim)
        self.chunk_images = None if chunk_images is None else int(chunk_images)
        self.device = torch.device(device)
        self.feat = torch.empty(self.n_images, self.dim, dtype=torch.float32, device=self.device)     # rows [0, n_encoded) are filled, in slot order
        self.slot_of = np.full(self.n_images, -1, dtype=np.int32)                                      # image -> slot, -1 = not encoded yet
        self.invalid = torch.zeros(1, dtype=torch.int32, device=self.device)                           # slots the head refused so far: read by check()
        self.n_encoded = 0              # images that went through encode_fn (= slots in use)
        self.n_requests = 0             # indices ensure() was asked for, repeats included

    def ensure(self, index):
        """index: host integer tensor of dataset indices (any shape, repeats allowed) -> their slots, int32, in the same shape.  Images without a slot
        are encoded once, in ascending image order, and appended."""
        index = torch.as_tensor(index)
        idx = index.reshape(-1).numpy().astype(np.int64, copy=False)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_images):
            raise IndexError(f'FeatureTable: image index outside [0, {self.n_images})')
        self.n_requests += idx.size
        missing = np.unique(idx[self.slot_of[idx] < 0])                # sorted, each image once
        step = self.chunk_images or max(1, missing.size)
        for lo in range(0, missing.size, step):
            part = missing[lo:lo + step]
            feat = self.encode_fn(torch.from_numpy(part))
            if tuple(feat.shape) != (part.size, self.dim):
                raise ValueError(f'FeatureTable: encode_fn returned {tuple(feat.shape)} for {part.size} images of dim {self.dim}')
            self.feat[self.n_encoded:self.n_encoded + part.size].copy_(feat)
            self.slot_of[part] = np.arange(self.n_encoded, self.n_encoded + part.size, dtype=np.int32)
            self.n_encoded += part.size
        return torch.from_numpy(self.slot_of[idx]).view(index.shape)

    def episodes(self, idx, way, shot, n_query, temp, method='cos'):
        """idx: host tensor of dataset indices, [G, ep_per_batch * way * (shot + n_query)] as the sampler yields them (class-major, the first `shot`
        of a class its shots) -> logits [E, way * n_query, way], acc [E], loss [E] with E = G * ep_per_batch: the bits of
        `engine.meta_baseline_forward` on the gathered images.  `ensure`, then one launch."""
        from .engine import ops
        idx = torch.as_tensor(idx)
        per_episode = way * (shot + n_query)
        if idx.numel() % per_episode:
            raise ValueError(f'episodes: {idx.numel()} indices are not a whole number of {way}-way {shot}+{n_query} episodes')
        slots = self.ensure(idx).view(-1, way, shot + n_query).to(self.device)       # (a blocking copy: the host array is a temporary)
        return ops.proto_head_gather(self.feat[:self.n_encoded], slots, shot, temp, self.invalid, method)

    def check(self):
        """One synchronisation, when the caller asks: raises if the head met a slot outside the filled part of the table."""
        n = int(self.invalid.item())
        if n:
            raise ValueError(f'fsvit: {n} episode index(es) pointed outside the {self.n_encoded} filled slots of the feature table; those episodes are NaN')

    def reset(self):
        """Forget every slot (the weights changed); the counters start again."""
        self.slot_of.fill(-1)
        self.invalid.zero_()
        self.n_encoded = self.n_requests = 0

    @classmethod
    def for_dataset(cls, model, dataset, chunk_images=None):
        """A table over `dataset` filled by the eval-mode encoder engine of `model` (a MetaBaseline): images come from `dataset.gather(index)`, or for a
        host dataset from stacking `dataset[i][0]`.  Refused (ValueError): a model in train mode (batch statistics, DropPath), and a dataset whose
        transform is not the deterministic eval transform - any `augment` but None / 'test', or `patches=` - which has no single feature per image."""
        from .datasets.transforms import DeviceTransform
        if model.training:
            raise ValueError('FeatureTable.for_dataset: the model is in train mode; a feature is a function of the image only in eval mode (model.eval())')
        transform = getattr(dataset, 'transform', None)
        if transform is not None and type(transform) is not DeviceTransform:
            raise ValueError(f'FeatureTable.for_dataset: the dataset applies {type(transform).__name__} - a random or multi-patch transform has no single '
                             "feature per image (build the dataset with augment=None / 'test' and patches=None)")
        engine = model.encoder.engine()
        device = engine.device

        def encode_fn(index):
            if model.training:
                raise RuntimeError('FeatureTable: the model went back to train mode; reset() the table and fill it in eval mode')
            if hasattr(dataset, 'gather'):
                x = dataset.gather(index)
            else:
                x = torch.stack([dataset[int(i)][0] for i in index]).to(device, non_blocking=True)
            return model.encoder.engine().forward(x)          # (re-packed by the encoder when a weight changed)

        return cls(encode_fn, len(dataset), engine.out_dim, device, chunk_images or engine.chunk_images)
