"""The host chain of the reference's udh/udh/dataset.py (SyntheticDataset.__getitem__) with Pillow and torch CPU ops: the reference of
tests/test_cpu_udh_data.py and tests/test_gpu_udh_data.py.  Pillow is the oracle of the resize; torchvision is not installed, so its
Resize(int) size rule and its CenterCrop origin come from masic_amd.udh_data.resize_geometry (restated, unpinned), and its ToTensor /
Normalize are the torch operations they are made of."""
import numpy as np
import torch
from PIL import Image

MEAN = torch.tensor([0.485, 0.456, 0.406]).mean().unsqueeze(0)          # dataset.py:10-11
STD = torch.tensor([0.229, 0.224, 0.225]).mean().unsqueeze(0)


def pil_resize(rgb, out_hw):
    """uint8 [H,W,3] -> uint8 [oh,ow,3] by Image.resize(BILINEAR); the picture itself when the size does not change"""
    oh, ow = int(out_hw[0]), int(out_hw[1])
    if (oh, ow) == tuple(rgb.shape[:2]):
        return np.ascontiguousarray(rgb)
    return np.asarray(Image.fromarray(np.ascontiguousarray(rgb)).resize((ow, oh), Image.BILINEAR))


def grey_picture(rgb, pic_size):
    """float32 [1,S,S]: mean_c(Normalize(ToTensor(CenterCrop(S)(Resize(S)(picture)))))"""
    from masic_amd.udh_data import resize_geometry
    S = int(pic_size)
    (oh, ow), (top, left) = resize_geometry(rgb.shape[:2], S)
    small = pil_resize(rgb, (oh, ow))[top:top + S, left:left + S]
    t = torch.from_numpy(np.array(small)).permute(2, 0, 1).float().div(255)
    t = t.contiguous().sub_(MEAN[:, None, None]).div_(STD[:, None, None])
    return t.mean(0, keepdim=True)


def item(left_rgb, right_rgb, x, y, pic_size, patch_size):
    """(img_a, img_b, patch_a, patch_b) of one item, float32 [1,.,.] CPU tensors"""
    p = int(patch_size)
    a, b = grey_picture(left_rgb, pic_size), grey_picture(right_rgb, pic_size)
    return a, b, a[:, y:y + p, x:x + p], b[:, y:y + p, x:x + p]
