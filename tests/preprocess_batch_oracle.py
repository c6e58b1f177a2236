"""ORACLE helper for ocr_preprocess_batch: the batch is nothing but oracle.preprocess_oracle.preprocess_image per image."""
import numpy as np

from oracle import preprocess_oracle as P


def preprocess_batch(images, target_w: int, target_h: int):
    """images: h x w x 4 u8 arrays -> (gray N x target_h x target_w u8, adjust N x 2 f64)."""
    gray = np.zeros((len(images), target_h, target_w), np.uint8)
    adj = np.zeros((len(images), 2), np.float64)
    for i, im in enumerate(images):
        gray[i], adj[i, 0], adj[i, 1] = P.preprocess_image(np.ascontiguousarray(im), target_w, target_h)
    return gray, adj
