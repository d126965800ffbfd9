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


def pil_bilinear_tables(in_size: int, out_size: int):
    """-> xmin [out] int32, count [out] int32, coef [out, ksize] int32 (zero padded)."""
    scale = float(in_size) / float(out_size)
    filterscale = max(scale, 1.0)
    support = filterscale                                    # bilinear support 1.0 * filterscale
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
            a = abs((x - center + 0.5) * inv)               # same association as Resample.c: (x + xmin - center + 0.5) * ss
            w = 1.0 - a if a < 1.0 else 0.0
            taps.append(w)
            total += w
        for j, w in enumerate(taps):
            if total != 0.0:
                w = w / total
            v = w * float(1 << PRECISION_BITS)
            coef[o, j] = int(v - 0.5) if w < 0 else int(v + 0.5)
        xmin[o], cnt[o] = lo, hi - lo
    return xmin, cnt, coef


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
        boxes, flips = torch.as_tensor(boxes).cpu(), torch.as_tensor(flips).cpu()
        if boxes.dim() != 2 or tuple(boxes.shape) != (n, 4) or flips.dim() != 1 or flips.numel() != n:
            raise ValueError(f'boxes must be [{n}, 4] and flips [{n}], got {tuple(boxes.shape)} and {tuple(flips.shape)}')
        boxes = boxes.to(torch.int64)
        i, j, h, w = boxes.unbind(1)
        if n and bool(((h <= 0) | (w <= 0) | (i < 0) | (j < 0) | (i + h > self.H) | (j + w > self.W)).any()):
            raise ValueError(f'crop box outside the {self.H} x {self.W} image or empty (rows are top, left, height, width)')
        return boxes.to(torch.int32).contiguous(), (flips != 0).to(torch.uint8).contiguous()

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
