"""The view form of the denoiser restated in numpy (pt_denoise_views, the denoised preview of a view frame): a batch is V
frames stacked as (V, H, W, ...), and a neighbour or tap counts only if it lies in the same view.  That is the single-frame filter applied
to every view on its own, so this module imports tests/denoise_ref.py and tests/preview_ref.py unchanged and calls them view by view."""
import numpy as np

from tests import denoise_ref, preview_ref


def denoise_views(rgba, features, **params):
    """denoise_ref.denoise of every view of a (V, H, W, 4) batch with its (V, H, W, 3, 4) features."""
    rgba, features = np.asarray(rgba, np.float32), np.asarray(features, np.float32)
    assert rgba.ndim == 4 and features.shape == rgba.shape[:3] + (3, 4)
    return np.stack([denoise_ref.denoise(rgba[v], features[v], **params) for v in range(len(rgba))])


def preview_denoise_views(rgba, features, samples, **params):
    """preview_ref.denoise (the hole-aware filter) of every view; samples is (V, H, W), 0 = a hole."""
    rgba, features, samples = np.asarray(rgba, np.float32), np.asarray(features, np.float32), np.asarray(samples)
    assert rgba.ndim == 4 and features.shape == rgba.shape[:3] + (3, 4) and samples.shape == rgba.shape[:3]
    return np.stack([preview_ref.denoise(rgba[v], features[v], samples[v], **params) for v in range(len(rgba))])
