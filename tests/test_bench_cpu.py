"""CPU: bench.dump_outputs on stand-in objects -- every array as float32 .npy, a seeded row sample of large batches."""
import os
import types

import numpy as np
import torch

import bench


class _Layer:
    def __init__(self, arrays):
        self.arrays = arrays

    def get_weights(self):
        return [a.copy() for a in self.arrays]


def _stand_ins(batch):
    blocks = [{"dense": _Layer([np.ones((880, 16), np.float32), np.zeros(16, np.float32)]), "bn": _Layer([np.ones(16, np.float32)] * 4)},
              {"dense": _Layer([np.ones((16, 10), np.float32), np.zeros(10, np.float32)]), "bn": None}]
    model = types.SimpleNamespace(_blocks=blocks, _loss_rows=torch.arange(batch + 5, dtype=torch.float32))
    pipe = types.SimpleNamespace(norms=torch.ones(3), feats=torch.arange(batch * 880, dtype=torch.float32).reshape(batch, 880))
    return pipe, model


def test_dump_outputs_small_batch(tmp_path):
    pipe, model = _stand_ins(64)
    n = bench.dump_outputs(str(tmp_path), pipe, model, 64, "product")
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(["block0_dense_kernel.npy", "block0_dense_bias.npy", "block0_bn_gamma.npy", "block0_bn_beta.npy",
                            "block0_bn_moving_mean.npy", "block0_bn_moving_variance.npy", "block1_dense_kernel.npy",
                            "block1_dense_bias.npy", "loss_rows.npy", "product_norms.npy", "features.npy"])
    assert all(np.load(tmp_path / f).dtype == np.float32 for f in files)
    np.testing.assert_array_equal(np.load(tmp_path / "features.npy"), pipe.feats.numpy())
    assert np.load(tmp_path / "loss_rows.npy").shape == (64,)
    assert n == sum(np.load(tmp_path / f).nbytes for f in files)


def test_dump_outputs_samples_rows_of_a_large_batch(tmp_path):
    batch = 8192
    pipe, model = _stand_ins(batch)
    bench.dump_outputs(str(tmp_path / "a"), pipe, model, batch, "none")
    bench.dump_outputs(str(tmp_path / "b"), pipe, model, batch, "none")
    assert not os.path.exists(tmp_path / "a" / "product_norms.npy")
    feats, rows = np.load(tmp_path / "a" / "features.npy"), np.load(tmp_path / "a" / "features_row_index.npy")
    assert feats.shape == (bench.DUMP_FEATURE_ROWS, 880) and rows.dtype == np.float64
    assert np.all(np.diff(rows) > 0) and rows.max() < batch
    np.testing.assert_array_equal(feats, pipe.feats.numpy()[rows.astype(np.int64)])
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "features_row_index.npy"))  # the same sample every run
