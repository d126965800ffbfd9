"""Host side of the device-resident eval transform: Pillow's BILINEAR resampling coefficient tables
(third-party arithmetic the reference reaches through torchvision.transforms.Resize on PIL images,
test_phase/datasets/mini_imagenet.py:50-51): for each output coordinate the first input index, the tap count and the
22-bit fixed-point taps, computed in double precision as Pillow's src/libImaging/Resample.c `precompute_coeffs` +
`normalize_coeffs_8bpc` do.  The HIP kernel behind fsvit_image_transform_gather applies them (two 8-bit passes).

Train-time augmentation `augment: resize` (sun_train_teacher/datasets/mini_imagenet.py:57-63): the host draws one crop box and one flip per
image (`random_resized_crop_boxes`, torchvision's RandomResizedCrop.get_params restated) and the kernel behind
fsvit_image_transform_rrc_gather computes each box's tables itself - the integers `pil_bilinear_tables(w, out)` gives - and resizes the crop."""
import math

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
IMAGENET_MEAN = (0.485, 0.456, 0.406)        # mini_imagenet.py:43-44
IMAGENET_STD = (0.229, 0.224, 0.225)


def _bilinear_filter(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic_filter(x):
    """Resample.c bicubic_filter, a = -0.5, with its association."""
    x = abs(x)
    if x < 1.0:
        return ((-0.5 + 2.0) * x - (-0.5 + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * -0.5
    return 0.0


FILTERS = {'bilinear': (0, _bilinear_filter, 1.0), 'bicubic': (1, _bicubic_filter, 2.0)}       # name -> (kernel code, filter, support)


def pil_resample_tables(in_size: int, out_size: int, filter: str = 'bilinear'):
    """-> xmin [out] int32, count [out] int32, coef [out, ksize] int32 (zero padded): `precompute_coeffs` + `normalize_coeffs_8bpc` for
    Pillow's BILINEAR (support 1) or BICUBIC (a = -0.5, support 2: negative taps, rounded with int(v - 0.5))."""
    _, filt, fsupport = FILTERS[filter]
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = fsupport * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    inv = 1.0 / filterscale
    xmin = np.zeros(out_size, np.int32)
    cnt = np.zeros(out_size, np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        taps = []
        total = 0.0
        for x in range(lo, hi):
            w = filt((x - center + 0.5) * inv)              # same association as Resample.c: (x + xmin - center + 0.5) * ss
            taps.append(w)
            total += w
        for j, w in enumerate(taps):
            if total != 0.0:
                w = w / total
            v = w * float(1 << PRECISION_BITS)
            coef[o, j] = int(v - 0.5) if w < 0 else int(v + 0.5)
        xmin[o], cnt[o] = lo, hi - lo
    return xmin, cnt, coef


def pil_bilinear_tables(in_size: int, out_size: int):
    """-> xmin [out] int32, count [out] int32, coef [out, ksize] int32 (zero padded)."""
    return pil_resample_tables(in_size, out_size, 'bilinear')


class DeviceTransform:
    """Resize((resize_h, resize_w)) -> CenterCrop(crop) -> ToTensor -> Normalize over uint8 images [N,H,W,3] resident on the GPU."""

    def __init__(self, in_hw, resize, crop, device, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        import ctypes as C
        self.H, self.W = in_hw
        self.RH, self.RW = (resize, resize) if isinstance(resize, int) else resize
        self.crop = crop
        self.y0 = int(round((self.RH - crop) / 2.0))          # torchvision F.center_crop
        self.x0 = int(round((self.RW - crop) / 2.0))
        th = pil_bilinear_tables(self.W, self.RW)
        tv = pil_bilinear_tables(self.H, self.RH)
        self.kh, self.kv = th[2].shape[1], tv[2].shape[1]
        self.device = torch.device(device)
        self._host_tables = th + tv                         # uploaded by the first call: constructing a dataset needs no GPU
        self.tab_h = self.tab_v = None
        self.mean = (C.c_float * 3)(*mean)
        self.std = (C.c_float * 3)(*std)

    def _upload(self):
        tabs = [torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in self._host_tables]
        self.tab_h, self.tab_v = tabs[:3], tabs[3:]

    def __call__(self, images: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
        from .. import _lib
        from ..engine import _ptr, _require_cuda, _stream_ptr
        _require_cuda(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_contiguous():
            raise ValueError('images must be a contiguous uint8 [N,H,W,3] tensor')
        if self.tab_h is None:
            self._upload()
        index = index.to(images.device, torch.int64).contiguous()
        B = index.numel()
        out = torch.empty(B, 3, self.crop, self.crop, dtype=torch.float32, device=images.device)
        lib = _lib.load()
        with torch.cuda.device(images.device):
            _lib.check(lib.fsvit_image_transform_gather(
                _ptr(images), self.H, self.W, _ptr(index), B, _ptr(self.tab_h[0]), _ptr(self.tab_h[1]), _ptr(self.tab_h[2]), self.kh,
                _ptr(self.tab_v[0]), _ptr(self.tab_v[1]), _ptr(self.tab_v[2]), self.kv, self.y0, self.x0, self.crop, self.crop,
                self.mean, self.std, _ptr(out), _stream_ptr(images.device)))
        return out


def random_resized_crop_boxes(n, H, W, generator, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.)):
    """n crop boxes (top i, left j, height h, width w) -> int32 [n, 4] CPU tensor: torchvision's RandomResizedCrop.get_params, vectorised over n.
    Up to 10 attempts per image: area = H*W*U(scale), r = exp(U(log ratio)), w = round(sqrt(area*r)), h = round(sqrt(area/r)); the first attempt
    with 0 < w <= W and 0 < h <= H is taken, with i uniform in [0, H-h] and j uniform in [0, W-w]; when all fail, the centre crop at the ratio
    clamped to `ratio`.  All draws come from `generator` (a fixed number per call, so a seed fixes the stream).

    The DISTRIBUTION is what is restated, not torchvision's random stream: torchvision is neither in the reference tree nor installed here, and
    the reference's own stream depends on DataLoader worker seeding anyway."""
    u = torch.rand(10, n, 2, generator=generator).double()                    # (area, ratio) of every attempt
    v = torch.rand(n, 2, generator=generator).double()                        # (i, j) of the accepted one
    area = H * W * (scale[0] + (scale[1] - scale[0]) * u[..., 0])
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    r = torch.exp(lo + (hi - lo) * u[..., 1])
    w = torch.round(torch.sqrt(area * r)).to(torch.int64)                     # [10, n]
    h = torch.round(torch.sqrt(area / r)).to(torch.int64)
    ok = (w > 0) & (w <= W) & (h > 0) & (h <= H)
    first = ok.to(torch.int8).argmax(0, keepdim=True)                         # first accepted attempt (0 where none is)
    any_ok = ok.any(0)
    w, h = w.gather(0, first)[0], h.gather(0, first)[0]
    i = torch.minimum((v[:, 0] * (H - h + 1)).floor().to(torch.int64), H - h)
    j = torch.minimum((v[:, 1] * (W - w + 1)).floor().to(torch.int64), W - w)
    in_ratio = float(W) / float(H)                                            # fallback: central crop
    if in_ratio < min(ratio):
        fw, fh = W, int(round(W / min(ratio)))
    elif in_ratio > max(ratio):
        fh, fw = H, int(round(H * max(ratio)))
    else:
        fw, fh = W, H
    fb = torch.tensor([(H - fh) // 2, (W - fw) // 2, fh, fw], dtype=torch.int64)
    boxes = torch.where(any_ok[:, None], torch.stack([i, j, h, w], 1), fb[None, :])
    return boxes.to(torch.int32).contiguous()


def _checked_boxes(n, boxes, flips, H, W):
    """Host validation of n crop boxes (top, left, height, width) and flips against an H x W image -> (int32 [n, 4], uint8 [n])."""
    boxes, flips = torch.as_tensor(boxes).cpu(), torch.as_tensor(flips).cpu()
    if boxes.dim() != 2 or tuple(boxes.shape) != (n, 4) or flips.dim() != 1 or flips.numel() != n:
        raise ValueError(f'boxes must be [{n}, 4] and flips [{n}], got {tuple(boxes.shape)} and {tuple(flips.shape)}')
    boxes = boxes.to(torch.int64)
    i, j, h, w = boxes.unbind(1)
    if n and bool(((h <= 0) | (w <= 0) | (i < 0) | (j < 0) | (i + h > H) | (j + w > W)).any()):
        raise ValueError(f'crop box outside the {H} x {W} image or empty (rows are top, left, height, width)')
    return boxes.to(torch.int32).contiguous(), (flips != 0).to(torch.uint8).contiguous()


class DeviceRandomResizedCrop:
    """RandomResizedCrop(out) -> RandomHorizontalFlip -> ToTensor -> Normalize over uint8 images [N,H,W,3] resident on the GPU (the reference's
    `augment: resize`).  Boxes and flips are drawn on the host from this object's generator, or passed in; `boxes` / `flips` keep the last call's."""

    def __init__(self, in_hw, out, device, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0):
        import ctypes as C
        self.H, self.W = in_hw
        self.out = int(out)
        self.device = torch.device(device)
        self.mean = (C.c_float * 3)(*mean)
        self.std = (C.c_float * 3)(*std)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.boxes = self.flips = None

    def manual_seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    def _checked(self, n, boxes, flips):
        return _checked_boxes(n, boxes, flips, self.H, self.W)

    def __call__(self, images: torch.Tensor, index: torch.Tensor, boxes=None, flips=None) -> torch.Tensor:
        from .. import _lib
        from ..engine import _ptr, _require_cuda, _stream_ptr
        B = index.numel()
        if (boxes is None) != (flips is None):
            raise ValueError('pass both boxes and flips, or neither')
        if boxes is None:
            boxes = random_resized_crop_boxes(B, self.H, self.W, self.generator)
            flips = torch.rand(B, generator=self.generator) < 0.5
        boxes, flips = self._checked(B, boxes, flips)                           # on the host, before anything reaches the device
        _require_cuda(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_contiguous():
            raise ValueError('images must be a contiguous uint8 [N,H,W,3] tensor')
        if tuple(images.shape[1:3]) != (self.H, self.W):
            raise ValueError(f'images are {tuple(images.shape[1:3])}, the transform was built for {(self.H, self.W)}')
        self.boxes, self.flips = boxes, flips.bool()
        index = index.to(images.device, torch.int64).contiguous()
        boxes_dev, flips_dev = boxes.to(images.device), flips.to(images.device)
        out = torch.empty(B, 3, self.out, self.out, dtype=torch.float32, device=images.device)
        lib = _lib.load()
        with torch.cuda.device(images.device):
            _lib.check(lib.fsvit_image_transform_rrc_gather(
                _ptr(images), self.H, self.W, _ptr(index), B, _ptr(boxes_dev), _ptr(flips_dev), self.out, self.out,
                self.mean, self.std, _ptr(out), _stream_ptr(images.device)))
        return out


# ---------------------------------------------------------------- SUN-D patch loaders (meta_tuning_sun_d/Models/dataloader/miniimagenet/{grid,sampling})
# Both are "crop box -> Pillow BILINEAR resize to out x out -> optional mirror -> ToTensor -> Normalize" per patch: fsvit_image_transform_rrc_gather with
# B * P rows (index repeated per patch, one box and one flip per row).
SUND_MEAN = tuple(x / 255.0 for x in (125.3, 123.0, 113.9))         # the statistics of the reference's SUN-D csv loaders
SUND_STD = tuple(x / 255.0 for x in (63.0, 62.1, 66.7))


def grid_location(size, ratio, num_grid):
    """get_grid_location (grid/mini_imagenet.py:78-97): the num_grid (lo, hi) extents along one axis of `size` pixels.  Even cells of
    int(size / num_grid) pixels, enlarged about their centres to int(size / num_grid * ratio) (float64, Python's operation order), clipped."""
    raw = int(size / num_grid)
    enl = int(size / num_grid * ratio)
    centre = raw // 2
    out = []
    for _ in range(num_grid):
        out.append((max(0, centre - enl // 2), min(size, centre + enl // 2)))
        centre += raw
    return out


def grid_boxes(H, W, ratio, num_grid):
    """The num_grid^2 boxes (top, left, height, width) of one pyramid level (get_pyramid, :116-131): rows (h) outer, columns (w) inner."""
    cols, rows = grid_location(W, ratio, num_grid), grid_location(H, ratio, num_grid)
    return [(t, l, b - t, r - l) for t, b in rows for l, r in cols]


class _DevicePatches:
    """B images -> [B, P, 3, out, out]: one launch of the random-resized-crop gather over B * P (index, box, flip) rows."""

    def __init__(self, in_hw, out, device, mean, std, seed):
        self._rrc = DeviceRandomResizedCrop(in_hw, out, device, mean=mean, std=std, seed=seed)
        self.H, self.W = in_hw
        self.out = int(out)
        self.device = self._rrc.device
        self.generator = self._rrc.generator
        self.boxes = self.flips = None

    def manual_seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    def draw(self, B):
        raise NotImplementedError

    def __call__(self, images: torch.Tensor, index: torch.Tensor, boxes=None, flips=None) -> torch.Tensor:
        """boxes int [B * P, 4] (top, left, height, width) and flips [B * P], image-major, or neither (drawn from this object's generator)."""
        index = torch.as_tensor(index).reshape(-1)
        B, P = index.numel(), self.n_patch
        if (boxes is None) != (flips is None):
            raise ValueError('pass both boxes and flips, or neither')
        if boxes is None:
            boxes, flips = self.draw(B)
        out = self._rrc(images, index.repeat_interleave(P), boxes, flips)
        self.boxes, self.flips = self._rrc.boxes, self._rrc.flips
        return out.view(B, P, 3, self.out, self.out)


class DevicePatchGrid(_DevicePatches):
    """The grid patches of SUN-D (grid/mini_imagenet.py:78-148): for every level n of `patch_list`, the n x n cells of the image enlarged by a
    ratio about their centres, each resized to out x out.  Patch order: levels in order; inside a level rows outer, columns inner.
    train=False (val / test): ratio = patch_ratio, no flips.  train=True: one ratio = 1 + 2 u, u ~ U[0, 1), per (image, level) - the reference draws
    once per get_pyramid call - and an independent flip with probability 0.5 per patch (the flip is inside the per-patch transform).  The
    distribution is restated, not the stream of Python's `random` (the stance of random_resized_crop_boxes)."""

    def __init__(self, in_hw, out, device, patch_list=(2, 3), patch_ratio=2.0, train=False, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0):
        super().__init__(in_hw, out, device, mean, std, seed)
        self.patch_list = tuple(int(n) for n in patch_list)
        if not self.patch_list or min(self.patch_list) < 1:
            raise ValueError(f'patch_list {patch_list!r}')
        self.patch_ratio, self.train = float(patch_ratio), bool(train)
        self.n_patch = sum(n * n for n in self.patch_list)

    def draw(self, B):
        if not self.train:
            one = [b for n in self.patch_list for b in grid_boxes(self.H, self.W, self.patch_ratio, n)]
            return torch.tensor(one, dtype=torch.int32).repeat(B, 1), torch.zeros(B * self.n_patch, dtype=torch.bool)
        u = torch.rand(B, len(self.patch_list), generator=self.generator, dtype=torch.float64)
        flips = torch.rand(B * self.n_patch, generator=self.generator) < 0.5
        boxes = [b for i in range(B) for k, n in enumerate(self.patch_list) for b in grid_boxes(self.H, self.W, 1 + 2 * float(u[i, k]), n)]
        return torch.tensor(boxes, dtype=torch.int32), flips


class DevicePatchSampler(_DevicePatches):
    """The sampled patches of SUN-D (sampling/mini_imagenet.py:41-58, the variant data_utils.set_up_datasets selects): num_patch independent
    RandomResizedCrop(out) + RandomHorizontalFlip per image, for every split - the reference samples random patches at evaluation time too."""

    def __init__(self, in_hw, out, device, num_patch=9, mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0):
        super().__init__(in_hw, out, device, mean, std, seed)
        self.n_patch = int(num_patch)
        if self.n_patch < 1:
            raise ValueError(f'num_patch {num_patch!r}')

    def draw(self, B):
        n = B * self.n_patch
        return random_resized_crop_boxes(n, self.H, self.W, self.generator), torch.rand(n, generator=self.generator) < 0.5


# ---------------------------------------------------------------- the distillation phase's strong / weak view pair
# (sun_meta_training/datasets/mini_imagenet.py:91-124, :194-204).  One int32 row per image tells the kernel behind fsvit_image_strong_weak what to do;
# the three factors are float32 bit patterns.
SW_STRONG, SW_ORDER, SW_FACTOR, SW_BLUR, SW_R, SW_WW, SW_FW, SW_SOLARIZE, SW_GRAY, SW_ERASE, SW_COLS = 0, 1, 4, 7, 8, 9, 10, 11, 12, 13, 17
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 0, 1, 2                  # values of the SW_ORDER columns; SW_FACTOR + op is that operation's factor
_PERMS = torch.tensor([[0, 1, 2], [0, 2, 1], [1, 0, 2], [1, 2, 0], [2, 0, 1], [2, 1, 0]], dtype=torch.int32)


def gaussian_blur_box(radius):
    """Pillow's ImageFilter.GaussianBlur(radius) = three box blurs per axis (BoxBlur.c): -> (r, ww, fw) int64 arrays, the integer box radius and the
    24-bit weights of the inner taps and of the two far taps, in the precisions of `_gaussian_blur_radius` and `ImagingLineBoxBlur8`."""
    f32 = np.float32
    rho = np.asarray(radius, np.float64).astype(f32)
    sigma2 = (rho * rho) / f32(3)
    L = np.sqrt(12.0 * sigma2.astype(np.float64) + 1.0).astype(f32)
    l = np.floor((L.astype(np.float64) - 1.0) / 2.0).astype(f32)
    a = (f32(2) * l + f32(1)) * (l * (l + f32(1)) - f32(3) * sigma2)
    a = a / (f32(6) * (sigma2 - (l + f32(1)) * (l + f32(1))))
    fr = l + a
    r = fr.astype(np.int64)
    ww = (f32(1 << 24) / (fr * f32(2) + f32(1))).astype(np.int64)
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def random_erase_boxes(n, H, W, generator, prob=0.25, area=(0.02, 1. / 3.), min_aspect=0.3):
    """timm's RandomErasing box (count 1), vectorised over n -> int32 [n, 4] (top, left, h, w), h = 0 where nothing is erased: with probability
    `prob`, up to 10 attempts of area = H*W*U(area), ratio = exp(U(log min_aspect, log 1/min_aspect)), h = round(sqrt(area*ratio)),
    w = round(sqrt(area/ratio)); the first with w < W and h < H is taken, top and left uniform integers in [0, H-h] and [0, W-w].  The distribution,
    not timm's stream (see random_resized_crop_boxes)."""
    u = torch.rand(10, n, 2, generator=generator).double()
    v = torch.rand(n, 3, generator=generator).double()                        # (apply, top, left)
    target = H * W * (area[0] + (area[1] - area[0]) * u[..., 0])
    lo, hi = math.log(min_aspect), math.log(1.0 / min_aspect)
    ratio = torch.exp(lo + (hi - lo) * u[..., 1])
    h = torch.round(torch.sqrt(target * ratio)).to(torch.int64)
    w = torch.round(torch.sqrt(target / ratio)).to(torch.int64)
    ok = (w < W) & (h < H) & (w > 0) & (h > 0)
    first = ok.to(torch.int8).argmax(0, keepdim=True)
    use = ok.any(0) & (v[:, 0] <= prob)
    h, w = h.gather(0, first)[0], w.gather(0, first)[0]
    top = torch.minimum((v[:, 1] * (H - h + 1)).floor().to(torch.int64), (H - h).clamp(min=0))
    left = torch.minimum((v[:, 2] * (W - w + 1)).floor().to(torch.int64), (W - w).clamp(min=0))
    box = torch.stack([top, left, h, w], 1)
    return torch.where(use[:, None], box, torch.zeros_like(box)).to(torch.int32).contiguous()


def strong_weak_table(n, generator, strong_prob=0.5, size=80):
    """The per-image parameter rows [n, SW_COLS] int32 of the strong view: strong flag (probability strong_prob), ColorJitter(0.4, 0.4, 0.4) - the
    order of brightness / contrast / saturation uniform over the 6 permutations, each factor U(0.6, 1.4) as float32 bits -, GaussianBlur(p = 0.5,
    radius U(0.1, 2)) as (flag, r, ww, fw), Solarization(0.5), RandomGrayscale(0.2), and the RandomErasing(0.25) box.  Every column is drawn for every
    image; the kernel ignores the colour columns of an image whose strong flag is 0 (the reference does not draw them then), never the erase box."""
    u = torch.rand(n, 8, generator=generator).double()
    perm = _PERMS[torch.randint(0, 6, (n,), generator=generator)]
    tab = torch.zeros(n, SW_COLS, dtype=torch.int32)
    tab[:, SW_STRONG] = (u[:, 0] <= strong_prob).to(torch.int32)
    tab[:, SW_ORDER:SW_ORDER + 3] = perm
    tab[:, SW_FACTOR:SW_FACTOR + 3] = (0.6 + 0.8 * u[:, 1:4]).to(torch.float32).view(torch.int32)
    tab[:, SW_BLUR] = (u[:, 4] <= 0.5).to(torch.int32)
    r, ww, fw = gaussian_blur_box((0.1 + 1.9 * u[:, 5]).numpy())
    tab[:, SW_R], tab[:, SW_WW], tab[:, SW_FW] = (torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32) for a in (r, ww, fw))
    tab[:, SW_SOLARIZE] = (u[:, 6] < 0.5).to(torch.int32)
    tab[:, SW_GRAY] = (u[:, 7] < 0.2).to(torch.int32)
    tab[:, SW_ERASE:SW_ERASE + 4] = random_erase_boxes(n, size, size, generator)
    return tab.contiguous()


def _checked_table(n, table, size):
    table = torch.as_tensor(table).cpu()
    if table.dim() != 2 or tuple(table.shape) != (n, SW_COLS) or table.dtype != torch.int32:
        raise ValueError(f'the parameter table must be int32 [{n}, {SW_COLS}], got {table.dtype} {tuple(table.shape)}')
    t = table.long()
    flags = t[:, [SW_STRONG, SW_BLUR, SW_SOLARIZE, SW_GRAY]]
    if bool(((flags != 0) & (flags != 1)).any()):
        raise ValueError('strong / blur / solarize / gray flags must be 0 or 1')
    if n and not bool((t[:, SW_ORDER:SW_ORDER + 3].sort(1).values == torch.arange(3)).all()):
        raise ValueError('the operation order must be a permutation of (0, 1, 2)')
    f = table[:, SW_FACTOR:SW_FACTOR + 3].contiguous().view(torch.float32)
    if not bool((torch.isfinite(f) & (f >= 0)).all()):
        raise ValueError('colour factors must be finite and non-negative')
    r, ww, fw = t[:, SW_R], t[:, SW_WW], t[:, SW_FW]
    if bool(((r < 0) | (r > 3) | (ww < 1) | ((2 * r + 1) * ww > (1 << 24)) | (fw != ((1 << 24) - (2 * r + 1) * ww) // 2)).any()):
        raise ValueError('blur box: need 0 <= r <= 3, ww >= 1, (2r+1) * ww <= 2^24 and fw = (2^24 - (2r+1) * ww) / 2')
    top, left, h, w = t[:, SW_ERASE:SW_ERASE + 4].unbind(1)
    if bool(((h < 0) | (w < 0) | (top < 0) | (left < 0) | (top + h > size) | (left + w > size) | ((h == 0) != (w == 0))).any()):
        raise ValueError(f'erase box outside the {size} x {size} view (columns are top, left, height, width; height = width = 0 for none)')
    return table.contiguous()


class DeviceStrongWeakPair:
    """The distillation phase's view pair over uint8 images [N,H,W,3] resident on the GPU: weak = RandomResizedCrop(out, BICUBIC) ->
    RandomHorizontalFlip; strong = weak, or with probability strong_prob ColorJitter -> GaussianBlur -> Solarization -> RandomGrayscale of it; both
    ToTensor + Normalize, RandomErasing('pixel') on the strong one.  Two launches per batch (fsvit_image_transform_rrc_u8, fsvit_image_strong_weak),
    bit-exact with Pillow up to the erase noise, which the kernel generates from `seed`.  `weak_randaug` is the probability of the weak view's
    RandomApply([RandAugment 'rand-m9-mstd0.5-inc1'], p) (the reference's 0.2; rand_augment_table): above 0 a third launch
    (fsvit_image_rand_augment) augments the drawn images in place between the two, so that strong and weak are both made from the result; at the
    default 0.0 nothing is drawn or launched for it.  All parameters are drawn on the host from this object's generator, or passed in; `params`
    keeps the last call's {'boxes', 'flips', 'table', 'seed'} (and 'randaug': (slots, table) when weak_randaug > 0), and
    `tf(images, index, params=tf.params)` replays it."""

    def __init__(self, in_hw, out=80, device='cuda', mean=IMAGENET_MEAN, std=IMAGENET_STD, strong_prob=0.5, seed=0, weak_randaug=0.0):
        import ctypes as C
        if int(out) != 80:
            raise NotImplementedError('fsvit: the strong / weak kernel is built for 80 x 80 views')
        self.H, self.W = in_hw
        self.out = int(out)
        self.device = torch.device(device)
        self.mean = (C.c_float * 3)(*mean)
        self.std = (C.c_float * 3)(*std)
        self.strong_prob = float(strong_prob)
        self.weak_randaug = float(weak_randaug)
        if not 0.0 <= self.weak_randaug <= 1.0:
            raise ValueError('weak_randaug is a probability')
        self.fill = (C.c_uint8 * 3)(*fill_colour(mean))
        self.generator = torch.Generator().manual_seed(int(seed))
        self.params = None

    def manual_seed(self, seed):
        self.generator.manual_seed(int(seed))
        return self

    def draw(self, n):
        boxes = random_resized_crop_boxes(n, self.H, self.W, self.generator)
        flips = torch.rand(n, generator=self.generator) < 0.5
        table = strong_weak_table(n, self.generator, self.strong_prob, self.out)
        seed = int(torch.randint(0, 1 << 62, (1,), generator=self.generator))
        params = {'boxes': boxes, 'flips': flips, 'table': table, 'seed': seed}
        if self.weak_randaug > 0:                                               # after every other draw: at 0 the stream is the one it always was
            params['randaug'] = rand_augment_table(n, self.generator, self.weak_randaug, self.out)
        return params

    @staticmethod
    def _checked_seed(seed):
        seed = int(seed)
        if not 0 <= seed < (1 << 64):
            raise ValueError('seed must fit 64 bits')
        return seed

    def _checked(self, n, params):
        boxes, flips = _checked_boxes(n, params['boxes'], params['flips'], self.H, self.W)
        randaug = _checked_randaug(n, *params['randaug']) if 'randaug' in params else None
        return boxes, flips, _checked_table(n, params['table'], self.out), self._checked_seed(params['seed']), randaug

    def _images(self, images, hw):
        from ..engine import _require_cuda
        _require_cuda(images)
        if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3 or not images.is_contiguous():
            raise ValueError('images must be a contiguous uint8 [N,H,W,3] tensor')
        if tuple(images.shape[1:3]) != tuple(hw):
            raise ValueError(f'images are {tuple(images.shape[1:3])}, expected {tuple(hw)}')

    # the launches, on arguments already validated
    def _crop_u8(self, images, index, boxes, flips, code):
        from .. import _lib
        from ..engine import _ptr, _stream_ptr
        B = index.numel()
        index = index.to(images.device, torch.int64).contiguous()
        boxes_dev, flips_dev = boxes.to(images.device), flips.to(images.device)
        out = torch.empty(B, self.out, self.out, 3, dtype=torch.uint8, device=images.device)
        with torch.cuda.device(images.device):
            _lib.check(_lib.load().fsvit_image_transform_rrc_u8(
                _ptr(images), self.H, self.W, _ptr(index), B, _ptr(boxes_dev), _ptr(flips_dev), self.out, self.out, code, _ptr(out),
                _stream_ptr(images.device)))
        return out

    def _strong_weak(self, views, table, seed):
        from .. import _lib
        from ..engine import _ptr, _stream_ptr
        B = views.shape[0]
        table_dev = table.to(views.device)
        weak = torch.empty(B, 3, self.out, self.out, dtype=torch.float32, device=views.device)
        strong = torch.empty_like(weak)
        with torch.cuda.device(views.device):
            _lib.check(_lib.load().fsvit_image_strong_weak(
                _ptr(views), B, self.out, self.out, _ptr(table_dev), SW_COLS, self.mean, self.std, seed, _ptr(weak), _ptr(strong),
                _stream_ptr(views.device)))
        return strong, weak

    def _rand_augment(self, views, slots, table):
        from .. import _lib
        from ..engine import _ptr, _stream_ptr
        slots_dev, table_dev = slots.to(views.device), table.to(views.device)
        with torch.cuda.device(views.device):
            _lib.check(_lib.load().fsvit_image_rand_augment(
                _ptr(views), views.shape[0], self.out, self.out, _ptr(slots_dev), slots.numel(), _ptr(table_dev), RA_COLS, self.fill,
                _stream_ptr(views.device)))
        return views

    def rand_augment(self, views, slots, table):
        """RandAugment IN PLACE on uint8 views [B, 80, 80, 3] on the GPU: image slots[k] gets the two operations of table[k] -> views."""
        slots, table = _checked_randaug(views.shape[0] if views.dim() == 4 else -1, slots, table)
        self._images(views, (self.out, self.out))
        return self._rand_augment(views, slots, table)

    def crop_u8(self, images, index, boxes, flips, filter='bicubic'):
        """Crop + Pillow resize (`filter`: 'bilinear' / 'bicubic') + flip -> uint8 [B, out, out, 3] on the GPU."""
        boxes, flips = _checked_boxes(index.numel(), boxes, flips, self.H, self.W)
        code = FILTERS[filter][0]
        self._images(images, (self.H, self.W))
        return self._crop_u8(images, index, boxes, flips, code)

    def strong_weak(self, views, table, seed=0):
        """uint8 weak views [B, 80, 80, 3] on the GPU + parameter table -> (strong, weak) float32 [B, 3, 80, 80]."""
        table = _checked_table(views.shape[0] if views.dim() == 4 else -1, table, self.out)
        seed = self._checked_seed(seed)
        self._images(views, (self.out, self.out))
        return self._strong_weak(views, table, seed)

    def __call__(self, images: torch.Tensor, index: torch.Tensor, params=None):
        B = index.numel()
        if params is None:
            params = self.draw(B)
        boxes, flips, table, seed, randaug = self._checked(B, params)          # once, on the host, before anything reaches the device
        self._images(images, (self.H, self.W))
        self.params = {'boxes': boxes, 'flips': flips.bool(), 'table': table, 'seed': seed}
        views = self._crop_u8(images, index, boxes, flips, FILTERS['bicubic'][0])
        if randaug is not None:
            self.params['randaug'] = randaug
            self._rand_augment(views, *randaug)
        return self._strong_weak(views, table, seed)


# ---------------------------------------------------------------- RandAugment: the weak view's RandomApply([rand-m9-mstd0.5-inc1], p = 0.2)
# (sun_meta_training/datasets/mini_imagenet.py:91-108) and the classifier phase's `cropaug` (sun_train_teacher/datasets/mini_imagenet.py, timm's
# create_transform).  One int32 row per AUGMENTED image tells the kernel behind fsvit_image_rand_augment what to do: RA_SLOTS operation slots of
# RA_OP_COLS columns each - a device operation code, one int32 argument (a table argument, or an enhance factor as float32 bits) and six float64
# affine coefficients as twelve int32.  timm's fifteen named operations map onto the twelve device codes here, on the host.
RA_SLOTS, RA_OP_COLS, RA_COLS = 2, 14, 28
RA_CODE, RA_ARG, RA_COEF = 0, 1, 2
(RA_NONE, RA_AFFINE, RA_INVERT, RA_POSTERIZE, RA_SOLARIZE, RA_SOLARIZE_ADD, RA_AUTOCONTRAST, RA_EQUALIZE, RA_COLOR, RA_CONTRAST, RA_BRIGHTNESS,
 RA_SHARPNESS) = range(12)
RA_FILL = tuple(min(255, round(255 * m)) for m in IMAGENET_MEAN)       # the reference's img_mean: (124, 116, 104)
RAND_INCREASING_OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'PosterizeIncreasing', 'SolarizeIncreasing', 'SolarizeAdd', 'ColorIncreasing',
                       'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing', 'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
RA_SIGNED = frozenset(('Rotate', 'ColorIncreasing', 'ContrastIncreasing', 'BrightnessIncreasing', 'SharpnessIncreasing', 'ShearX', 'ShearY',
                       'TranslateXRel', 'TranslateYRel'))
_RA_ENHANCE = {'ColorIncreasing': RA_COLOR, 'ContrastIncreasing': RA_CONTRAST, 'BrightnessIncreasing': RA_BRIGHTNESS,
               'SharpnessIncreasing': RA_SHARPNESS}
_RA_TABLE_ARG = {RA_POSTERIZE: (0, 8), RA_SOLARIZE: (0, 256), RA_SOLARIZE_ADD: (0, 255)}       # inclusive argument ranges


def fill_colour(mean):
    """The reference's img_mean: min(255, round(255 * mean)) per channel."""
    return tuple(min(255, int(round(255 * float(m)))) for m in mean)


def rotate_matrix(degrees, w, h):
    """The six AFFINE coefficients Pillow's Image.rotate(degrees) hands to Image.transform for a w x h image (centre (w/2, h/2), no expansion), or
    None when degrees % 360 == 0, where Image.rotate returns a copy.  (Its transpose shortcuts at 90 / 180 / 270 are out of RandAugment's +-30.)"""
    angle = degrees % 360.0
    if angle == 0:
        return None
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def rand_augment_op(name, magnitude, negate=False, size=80, translate_pct=0.45):
    """One operation slot (int32 [RA_OP_COLS]) for timm's operation `name` of the 'increasing' set at `magnitude` (0..10): timm's level maps
    (auto_augment.py `_*_level_to_arg`) and the matrices its PIL calls build, in Python float64."""
    m = float(magnitude) / 10.0
    sign = -1.0 if negate else 1.0
    code, arg, coef = RA_NONE, 0, None
    if name == 'AutoContrast':
        code = RA_AUTOCONTRAST
    elif name == 'Equalize':
        code = RA_EQUALIZE
    elif name == 'Invert':
        code = RA_INVERT
    elif name == 'Rotate':
        coef = rotate_matrix(sign * (m * 30.0), size, size)
    elif name == 'PosterizeIncreasing':
        code, arg = RA_POSTERIZE, 4 - int(m * 4)
    elif name == 'SolarizeIncreasing':
        code, arg = RA_SOLARIZE, 256 - int(m * 256)
    elif name == 'SolarizeAdd':
        code, arg = RA_SOLARIZE_ADD, min(128, int(m * 110))
    elif name in _RA_ENHANCE:
        code = _RA_ENHANCE[name]
        arg = int(np.asarray([max(0.1, 1.0 + sign * (m * 0.9))], np.float32).view(np.int32)[0])
    elif name == 'ShearX':
        coef = (1, sign * (m * 0.3), 0, 0, 1, 0)
    elif name == 'ShearY':
        coef = (1, 0, 0, sign * (m * 0.3), 1, 0)
    elif name == 'TranslateXRel':
        coef = (1, 0, sign * (m * translate_pct) * size, 0, 1, 0)
    elif name == 'TranslateYRel':
        coef = (1, 0, 0, 0, 1, sign * (m * translate_pct) * size)
    else:
        raise ValueError(f'unknown RandAugment operation {name!r}')
    op = np.zeros(RA_OP_COLS, np.int32)
    if coef is not None:
        code = RA_AFFINE
        op[RA_COEF:RA_COEF + 12] = np.asarray(coef, np.float64).view(np.int32)
    op[RA_CODE], op[RA_ARG] = code, arg
    return op


def rand_augment_draw(n, generator, apply_prob, magnitude=9, magnitude_std=0.5, num_layers=RA_SLOTS):
    """The random part of rand_augment_table, a fixed number of draws per call: 'apply' [n] (RandomApply), and per layer 'op' (index into
    RAND_INCREASING_OPS, uniform with replacement), 'on' (each operation's own probability 0.5), 'raw' (N(magnitude, magnitude_std)),
    'magnitude' (raw clipped to [0, 10]) and 'negate' (the sign of the signed operations)."""
    u = torch.rand(n, 1 + 2 * num_layers, generator=generator).double()
    op = torch.randint(0, len(RAND_INCREASING_OPS), (n, num_layers), generator=generator)
    raw = magnitude + magnitude_std * torch.randn(n, num_layers, generator=generator).double()
    return {'apply': u[:, 0] < apply_prob, 'op': op, 'on': u[:, 1:1 + num_layers] < 0.5, 'negate': u[:, 1 + num_layers:] < 0.5, 'raw': raw,
            'magnitude': raw.clamp(0.0, 10.0)}


def rand_augment_table(n, generator, apply_prob, size=80, magnitude=9, magnitude_std=0.5, num_layers=RA_SLOTS, translate_pct=0.45):
    """-> (slots int32 [k], table int32 [k, RA_COLS]): timm's RandAugment 'rand-m9-mstd0.5-inc1' drawn for n images.  With probability `apply_prob`
    an image is augmented: `num_layers` operations uniform WITH replacement from the 15 of RAND_INCREASING_OPS, each applied with probability 0.5 at
    its own magnitude clip(N(magnitude, magnitude_std), 0, 10), the signed ones negated with probability 0.5.  `slots` lists, strictly increasing,
    the images with at least one applied operation; a skipped operation is an RA_NONE slot.  The fill colour of the geometric operations is not
    part of the table: it goes with the call (fill_colour(mean), the reference's img_mean).

    timm is neither in the reference tree nor installed here, so this is timm's published algorithm (auto_augment.py: RandAugment, AugmentOp,
    `_RAND_INCREASING_TRANSFORMS`, the `_*_level_to_arg` maps) restated and its parity is UNPINNED: no test compares it with timm itself.  As
    elsewhere in this file the distribution is what is restated, not timm's random stream."""
    if num_layers != RA_SLOTS:
        raise NotImplementedError(f'fsvit: the RandAugment kernel applies {RA_SLOTS} operation slots')
    d = rand_augment_draw(n, generator, apply_prob, magnitude, magnitude_std, num_layers)
    listed = (d['apply'][:, None] & d['on']).any(1).nonzero()[:, 0]
    table = np.zeros((listed.numel(), RA_COLS), np.int32)
    op, on, mag, neg = d['op'].tolist(), d['on'].tolist(), d['magnitude'].tolist(), d['negate'].tolist()
    for k, b in enumerate(listed.tolist()):
        for s in range(num_layers):
            if on[b][s]:
                table[k, s * RA_OP_COLS:(s + 1) * RA_OP_COLS] = rand_augment_op(RAND_INCREASING_OPS[op[b][s]], mag[b][s], neg[b][s], size, translate_pct)
    return listed.to(torch.int32).contiguous(), torch.from_numpy(table)


def _checked_randaug(n, slots, table):
    """Host validation of a RandAugment (slots, table) pair for a batch of n images -> (int32 [k], int32 [k, RA_COLS])."""
    slots, table = torch.as_tensor(slots).cpu(), torch.as_tensor(table).cpu()
    if slots.dim() != 1 or slots.dtype != torch.int32:
        raise ValueError(f'slots must be a 1-d int32 tensor, got {slots.dtype} {tuple(slots.shape)}')
    k = slots.numel()
    if table.dim() != 2 or tuple(table.shape) != (k, RA_COLS) or table.dtype != torch.int32:
        raise ValueError(f'the RandAugment table must be int32 [{k}, {RA_COLS}], got {table.dtype} {tuple(table.shape)}')
    s = slots.long()
    if k and (int(s[0]) < 0 or int(s[-1]) >= n or bool((s[1:] <= s[:-1]).any())):
        raise ValueError(f'slots must be strictly increasing image indices in [0, {n})')
    ops = table.contiguous().view(k * RA_SLOTS, RA_OP_COLS)
    code, arg = ops[:, RA_CODE].long(), ops[:, RA_ARG]
    if bool(((code < RA_NONE) | (code > RA_SHARPNESS)).any()):
        raise ValueError(f'operation codes must be in [{RA_NONE}, {RA_SHARPNESS}]')
    coef = ops[:, RA_COEF:RA_COEF + 12].contiguous().view(torch.float64)[code == RA_AFFINE]
    if not bool(torch.isfinite(coef).all()):
        raise ValueError('affine coefficients must be finite')
    f = arg.contiguous().view(torch.float32)[(code >= RA_COLOR) & (code <= RA_SHARPNESS)]
    if not bool((torch.isfinite(f) & (f >= 0)).all()):
        raise ValueError('enhance factors must be finite and non-negative')
    for c, (lo, hi) in _RA_TABLE_ARG.items():
        a = arg[code == c]
        if bool(((a < lo) | (a > hi)).any()):
            raise ValueError(f'the argument of operation code {c} must be in [{lo}, {hi}]')
    return slots.contiguous(), table.contiguous()


class DeviceRandAugCrop:
    """The classifier phase's timm pipeline (the reference's `augment: cropaug`, sun_train_teacher/datasets/mini_imagenet.py: timm's
    create_transform with auto_augment 'rand-m9-mstd0.5-inc1', which drops its colour jitter) over uint8 images [N,H,W,3] resident on the GPU:
    RandomResizedCrop(out, BICUBIC) -> RandomHorizontalFlip -> RandAugment (always applied) -> ToTensor -> Normalize -> RandomErasing(0.25,
    'pixel') -> float32 [B, 3, 80, 80].  It is the view pair's three launches with the strong flag 0 everywhere: the result is the pair's `strong`
    output (the un-jittered view, erased); its `weak` store is made and dropped.  Same `draw` / `params` / replay surface as DeviceStrongWeakPair
    (`pair`, which does the work)."""

    def __init__(self, in_hw, out=80, device='cuda', mean=IMAGENET_MEAN, std=IMAGENET_STD, seed=0):
        self.pair = DeviceStrongWeakPair(in_hw, out, device, mean, std, strong_prob=0.0, seed=seed, weak_randaug=1.0)
        self.H, self.W, self.out, self.device = self.pair.H, self.pair.W, self.pair.out, self.pair.device
        self.mean, self.std, self.fill, self.generator = self.pair.mean, self.pair.std, self.pair.fill, self.pair.generator

    @property
    def params(self):
        return self.pair.params

    def manual_seed(self, seed):
        self.pair.manual_seed(seed)
        return self

    def draw(self, n):
        params = self.pair.draw(n)
        params['table'][:, SW_STRONG] = 0                                       # (u <= 0 has probability 2^-24 per image)
        return params

    def __call__(self, images: torch.Tensor, index: torch.Tensor, params=None) -> torch.Tensor:
        if params is None:
            params = self.draw(index.numel())
        elif 'randaug' not in params:
            raise ValueError("params needs 'randaug': (slots, table)")
        return self.pair(images, index, params)[0]
