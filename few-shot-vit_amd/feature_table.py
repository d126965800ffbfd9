"""FeatureTable: every image of a dataset goes through the encoder once, the episodes read their rows through the sampler's index table.

The reference's evaluation (test_phase/test_few_shot.py:76-92) encodes every image an episode draws: 2000 five-way episodes over a 12 000-image
test split are 160 000 (1-shot) or 200 000 (5-shot) encoder passes.  In eval mode the transform is deterministic (Resize -> CenterCrop), BatchNorm
uses its running statistics and the engines give the same bits for an image whatever launch it sits in, so the feature of image i is a function
of i alone.  The table keeps it: `ensure` encodes the images it has not seen (ascending image order, the engine's chunks) and hands back slot numbers,
`episodes` runs the episode head over those slots in one launch (fsvit_proto_head_gather, head.hip) - no image tensor, no feature copy; `auc` does
the same for the `--sauc` reduction (fsvit_proto_auc_gather, proto_bank.hip) and encodes only the images that reduction reads.

TokenTable does the same for the DeepEMD head (eval_deepemd -feature_cache, train_deepemd -eval_feature_cache): its rows are whole node sets - the
token map of an image, or the features of its grid patches - with the head's node preparation done once per image, and `logits` runs the
transportation problems over slot numbers (fsvit_emd_head_gather, emd_head.hip).

The bookkeeping (`slot_of`, the counters, the order of the encoder calls) is host-side numpy, shared by both tables (_SlotTable), and does not look
at the device; only `episodes` / `logits` and `for_dataset` need the GPU.  The tables do not watch the weights: call `reset()` when they change."""
import numpy as np
import torch

from .episodic import gather_images


class _SlotTable:
    """The host bookkeeping both tables share: image -> slot, the counters, the order and the size of the encoder calls.  A subclass keeps the rows
    (`_store`) and runs its head over the slots."""

    _what = 'table'

    def __init__(self, encode_fn, n_images, device, chunk_images=None):
        name = type(self).__name__
        if int(n_images) < 1:
            raise ValueError(f'{name} needs n_images >= 1')
        if chunk_images is not None and int(chunk_images) < 1:
            raise ValueError('chunk_images >= 1')
        self.encode_fn = encode_fn
        self.n_images = int(n_images)
        self.chunk_images = None if chunk_images is None else int(chunk_images)
        self.device = torch.device(device)
        self.slot_of = np.full(self.n_images, -1, dtype=np.int32)                                      # image -> slot, -1 = not encoded yet
        self.invalid = torch.zeros(1, dtype=torch.int32, device=self.device)                           # slots the head refused so far: read by check()
        self.n_encoded = 0              # images that went through encode_fn (= slots in use)
        self.n_requests = 0             # indices ensure() was asked for, repeats included

    def _store(self, lo, rows, n):
        """Keep what encode_fn returned for `n` images as the slots [lo, lo + n); raises ValueError on a wrong shape."""
        raise NotImplementedError

    def ensure(self, index):
        """index: host integer tensor of dataset indices (any shape, repeats allowed) -> their slots, int32, in the same shape.  Images without a slot
        are encoded once, in ascending image order, and appended."""
        index = torch.as_tensor(index)
        idx = index.reshape(-1).numpy().astype(np.int64, copy=False)
        if idx.size and (idx.min() < 0 or idx.max() >= self.n_images):
            raise IndexError(f'{type(self).__name__}: image index outside [0, {self.n_images})')
        self.n_requests += idx.size
        missing = np.unique(idx[self.slot_of[idx] < 0])                # sorted, each image once
        step = self.chunk_images or max(1, missing.size)
        for lo in range(0, missing.size, step):
            part = missing[lo:lo + step]
            self._store(self.n_encoded, self.encode_fn(torch.from_numpy(part)), part.size)
            self.slot_of[part] = np.arange(self.n_encoded, self.n_encoded + part.size, dtype=np.int32)
            self.n_encoded += part.size
        return torch.from_numpy(self.slot_of[idx]).view(index.shape)

    def check(self):
        """One synchronisation, when the caller asks: raises if the head met a slot outside the filled part of the table."""
        n = int(self.invalid.item())
        if n:
            raise ValueError(f'fsvit: {n} episode index(es) pointed outside the {self.n_encoded} filled slots of the {self._what}; those episodes are NaN')

    def reset(self):
        """Forget every slot (the weights changed); the counters start again."""
        self.slot_of.fill(-1)
        self.invalid.zero_()
        self.n_encoded = self.n_requests = 0


class FeatureTable(_SlotTable):

    _what = 'feature table'

    def __init__(self, encode_fn, n_images, dim, device, chunk_images=None):
        """encode_fn(index) -> [len(index), dim] features on `device` for a sorted 1-d int64 host tensor of image indices; it is handed at most
        `chunk_images` indices per call (None: no limit)."""
        if int(n_images) < 1 or int(dim) < 1:
            raise ValueError('FeatureTable needs n_images >= 1 and dim >= 1')
        super().__init__(encode_fn, n_images, device, chunk_images)
        self.dim = int(dim)
        self.feat = torch.empty(self.n_images, self.dim, dtype=torch.float32, device=self.device)     # rows [0, n_encoded) are filled, in slot order

    def _store(self, lo, feat, n):
        if tuple(feat.shape) != (n, self.dim):
            raise ValueError(f'FeatureTable: encode_fn returned {tuple(feat.shape)} for {n} images of dim {self.dim}')
        self.feat[lo:lo + n].copy_(feat)

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

    def auc(self, idx, shot, n_query):
        """The `--sauc` reduction.  idx: host tensor of dataset indices of 2-way episodes, [G, ep_per_batch * 2 * (shot + n_query)] as the sampler yields
        them (class-major) -> auc [E], E = G * ep_per_batch: the bits of `ops.proto_auc` on the gathered images.  Only what the reduction reads is
        encoded - the `shot` shots of class 0 and all 2 * n_query queries, class 0's (the positives) first; the shots of class 1 are never touched
        (the reference scores against `x_shot[:, 0]`).  `ensure`, then one launch."""
        from .engine import ops
        idx = torch.as_tensor(idx)
        per_episode = 2 * (shot + n_query)
        if idx.numel() % per_episode:
            raise ValueError(f'auc: {idx.numel()} indices are not a whole number of 2-way {shot}+{n_query} episodes')
        idx = idx.reshape(-1, 2, shot + n_query)
        E = idx.shape[0]
        used = torch.cat([idx[:, 0, :shot].reshape(-1), idx[:, :, shot:].reshape(-1)])
        slots = self.ensure(used).to(self.device)                     # (a blocking copy: the host array is a temporary)
        return ops.proto_auc_gather(self.feat[:self.n_encoded], slots[:E * shot].view(E, shot), slots[E * shot:].view(E, 2 * n_query), self.invalid)

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
            return model.encoder.engine().forward(gather_images(dataset, index, device))        # (re-packed by the encoder when a weight changed)

        return cls(encode_fn, len(dataset), engine.out_dim, device, chunk_images or engine.chunk_images)


class TokenTable(_SlotTable):
    """The DeepEMD head's table: per image the node set `tok` [N, C] (the token map, or the pooled features of its grid patches), and what the head's
    node preparation makes of it - `xhat` (channel-centred, L2-normalised nodes) and `pooled` (token mean) -, prepared once when the image is appended
    (fsvit_emd_table_prep).  `logits` runs the transportation problems of whole episodes over slot numbers (fsvit_emd_head_gather): the bits of
    `DeepEMD.forward` on the gathered images.  Forward-only.  Memory: fp32 `tok` + `xhat` of 12 000 images x 25 tokens x 512 channels are 1.2 GB; the
    arrays are allocated when the first chunk tells N and C."""

    _what = 'token-map table'

    def __init__(self, encode_fn, n_images, device, chunk_images=None, prep_fn=None):
        """encode_fn(index) -> [len(index), N, C] node sets on `device` for a sorted 1-d int64 host tensor of image indices, at most `chunk_images`
        per call.  prep_fn(tok, xhat, pooled) fills xhat / pooled for the rows of one chunk (None: ops.emd_table_prep)."""
        super().__init__(encode_fn, n_images, device, chunk_images)
        self.prep_fn = prep_fn
        self.tok = self.xhat = self.pooled = None          # [n_images, N, C] x 2, [n_images, C]; rows [0, n_encoded) are filled, in slot order

    def _store(self, lo, tok, n):
        if tok.dim() != 3 or tok.shape[0] != n or (self.tok is not None and tuple(tok.shape[1:]) != tuple(self.tok.shape[1:])):
            raise ValueError(f'TokenTable: encode_fn returned {tuple(tok.shape)} for {n} images' +
                             ('' if self.tok is None else f' of {self.tok.shape[1]} nodes x {self.tok.shape[2]} channels'))
        if self.tok is None:
            N, C = tok.shape[1:]
            self.tok = torch.empty(self.n_images, N, C, dtype=torch.float32, device=self.device)
            self.xhat = torch.empty_like(self.tok)
            self.pooled = torch.empty(self.n_images, C, dtype=torch.float32, device=self.device)
        self.tok[lo:lo + n].copy_(tok)
        prep = self.prep_fn
        if prep is None:
            from .engine import ops
            prep = ops.emd_table_prep
        prep(self.tok[lo:lo + n], self.xhat[lo:lo + n], self.pooled[lo:lo + n])

    def logits(self, idx, way, shot, n_query, model):
        """idx: host tensor of dataset indices, E * way * (shot + n_query) of them as the sampler yields them (class-major, the first `shot` of a class
        its shots) -> logits [E, way * n_query, way]: the bits of `model(x_shot, x_query)` (a DeepEMD in eval mode) on the gathered images.  1-shot: one
        launch over slots.  More shots: `model.get_sfc` on the support maps gathered from `tok` (the fine-tune the dense route runs, with the same
        generator and call order), then one launch with the SFC as the dense class side.  The solver's status goes to `model.add_status`."""
        from .engine import ops
        idx = torch.as_tensor(idx)
        per_class = shot + n_query
        if idx.numel() % (way * per_class):
            raise ValueError(f'logits: {idx.numel()} indices are not a whole number of {way}-way {shot}+{n_query} episodes')
        slots = self.ensure(idx).view(-1, way, per_class).to(self.device)            # (a blocking copy: the host array is a temporary)
        E = slots.shape[0]
        query_slots = slots[:, :, shot:].reshape(E, way * n_query)
        n = self.n_encoded
        tok, xhat, pooled = self.tok[:n], self.xhat[:n], self.pooled[:n]
        if shot == 1:
            logits, status = ops.emd_head_gather(tok, xhat, pooled, query_slots, model.temperature, self.invalid, proto_slots=slots[:, :, 0])
        else:
            sfc = model.get_sfc(tok[slots[:, :, :shot].long()], generator=model.sfc_generator)
            logits, status = ops.emd_head_gather(tok, xhat, pooled, query_slots, model.temperature, self.invalid, proto_tok=sfc)
        model.add_status(status)
        return logits

    @classmethod
    def for_dataset(cls, model, dataset, chunk_images=None):
        """A table over `dataset` filled by `model.encode` (a DeepEMD) in eval mode: `-deepemd fcn` keeps the token map of every image, `-deepemd grid`
        the pooled feature of each of its deterministic grid patches.  Images come from `dataset.gather(index)`, or for a host dataset from stacking
        `dataset[i][0]`.  Refused (ValueError), because none has a single node set per image: a model in train mode, `patches='sampling'`, the grid
        loader with `patch_train=True`, any random `augment`; also a dataset whose loader is not the one the model's `deepemd` mode reads."""
        from .datasets.transforms import DevicePatchGrid, DeviceTransform
        if model.training:
            raise ValueError('TokenTable.for_dataset: the model is in train mode; a node set is a function of the image only in eval mode (model.eval())')
        transform = getattr(dataset, 'transform', None)
        grid = type(transform) is DevicePatchGrid
        if grid and transform.train:
            raise ValueError('TokenTable.for_dataset: the grid loader with patch_train=True draws random ratios and flips - no single node set per image')
        if transform is not None and not grid and type(transform) is not DeviceTransform:
            raise ValueError(f'TokenTable.for_dataset: the dataset applies {type(transform).__name__} - a random transform has no single node set per '
                             "image (build the dataset with augment=None / 'test' and patches=None or 'grid')")
        patches = model.deepemd != 'fcn'
        if model.deepemd == 'sampling' or patches != grid:
            raise ValueError(f'TokenTable.for_dataset: a model with deepemd={model.deepemd!r} over a dataset ' +
                             ('of grid patches' if grid else 'of whole images') + ' - no single node set per image')
        engine = model.encoder.engine()
        device = engine.device
        per_image = transform.n_patch if grid else 1

        def encode_fn(index):
            if model.training:
                raise RuntimeError('TokenTable: the model went back to train mode; reset() the table and fill it in eval mode')
            with torch.no_grad():
                return model.encode(gather_images(dataset, index, device), patches)      # (the engine is re-packed by the encoder when a weight changed)

        # model.encode reads the token map of the encoder's last launch: a chunk must fit one launch of the engine
        return cls(encode_fn, len(dataset), device, chunk_images or max(1, engine.chunk_images // per_image))
