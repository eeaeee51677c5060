"""Golden fixture for the Gaussian filter, produced by running the REFERENCE's own code on CPU (needs the reference
checkout, as make_golden.py does; the tests read only the recorded file):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gauss.py

  gauss.npz -- functional.py:44-51 generate_gaussian_1d_kernel(sigma, 4.0) for six sigmas, intensity_transforms.py:117-142
               GaussianSmooth.apply_to_image for four of them on the (12, 20, 28) volume of augment.npz, and the chain
               of models.py:66-74 with the commented-out GaussianSmooth (:68) switched on -- GaussianAddictive ->
               BoxMaskOut -> GaussianSmooth(0.45) -> Flip -> CropAndResize -- through the reference's classes with the
               FIXED parameters and the noise seed of make_golden_f.augment_case(), every intermediate saved.
Only data is committed -- never reference source.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
from make_golden import import_ref_models  # noqa: E402  (also puts the reference on sys.path)

rm = import_ref_models()
import functional as ref_func              # noqa: E402
import intensity_transforms as ref_it      # noqa: E402

TAP_SIGMAS = (0.1, 0.3, 0.45, 0.6, 1.0, 2.0)
SMOOTH_SIGMAS = (0.3, 0.45, 0.6, 2.0)
CHAIN_SIGMA = 0.45


def smooth(img, sigma):
    gs = ref_it.GaussianSmooth(p=1.0, always_apply=True, sigma=(0.3, 0.6))
    gs.params = {"sigma": sigma, "truncate": gs.truncate}
    return gs.apply_to_image(img.clone())


def gauss_case():
    g = torch.Generator().manual_seed(123)
    img = torch.randn(12, 20, 28, generator=g)                # augment_case()'s image
    rec = dict(image=img.numpy(), tap_sigmas=np.array(TAP_SIGMAS), smooth_sigmas=np.array(SMOOTH_SIGMAS))
    for i, s in enumerate(TAP_SIGMAS):
        rec[f"taps_{i}"] = ref_func.generate_gaussian_1d_kernel(s, 4.0).numpy()
    for i, s in enumerate(SMOOTH_SIGMAS):
        rec[f"smooth_{i}"] = smooth(img, s).numpy()
    # the chain, parameters and noise seed as in make_golden_f.augment_case()
    ga = rm.GaussianAddictive(p=1.0, always_apply=True)
    ga.params = {"sigma": 0.045}
    torch.manual_seed(4242)                                   # the transform draws torch.randn(data.shape) itself
    a1 = ga.apply_to_image(img.clone())
    bm = rm.BoxMaskOut(p=1.0, always_apply=True, n_masks=(1, 10))
    centers = [(0.3, 0.5, 0.7), (0.62, 0.25, 0.41), (0.8, 0.8, 0.2)]
    sizes = [(0.3, 0.2, 0.25), (0.2, 0.35, 0.1), (0.5, 0.1, 0.3)]
    bm.params = {"n_masks": 3, "mask_centers": centers, "mask_sizes": sizes}
    a2 = bm.apply_to_image(a1)
    a3 = smooth(a2, CHAIN_SIGMA)
    fl = rm.Flip(1.0, True, dim=(1, 3))
    fl.params = {"combs": [2, 0]}
    a4 = fl.apply_to_image(a3)
    cr = rm.CropAndResize(1.0, True, (0.45, 0.55), (0.95, 1.0), align_corners=True)
    cc, cs = (0.47, 0.53, 0.5), (0.96, 0.99, 0.95)
    cr.params = {"crop_center": cc, "crop_size": cs}
    a5 = cr.apply_to_image(a4)
    rec.update(noise_sigma=np.array(0.045), noise_seed=np.array(4242), box_centers=np.array(centers),
               box_sizes=np.array(sizes), chain_sigma=np.array(CHAIN_SIGMA), flip_dims=np.array([2, 0]),
               crop_center=np.array(cc), crop_size=np.array(cs), after_noise=a1.numpy(), after_box=a2.numpy(),
               after_smooth=a3.numpy(), after_flip=a4.numpy(), after_crop=a5.numpy())
    return rec


if __name__ == "__main__":
    torch.set_num_threads(8)
    np.savez_compressed(os.path.join(HERE, "gauss.npz"), **gauss_case())
    print("wrote gauss.npz")
