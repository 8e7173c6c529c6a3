"""MI355X-native Gaussian-Process residual model for the quadrotor GP-MPC workspace.

Host side in Python (the reference's language) over the libgpk C ABI (hand-written gfx950 HIP
kernels).  Public surface mirrors the reference's seams:

    GaussianProcessRegressor, RBF, WhiteKernel, ConstantKernel   (estimator seam, gpr.py / kernels.py)
    SimpleQuadrotorGP, SimpleGPEnhancedMPC                        (model seam, simple_gp.py)
    GaussianProcess                                               (ROS-package GP, package_gp.py)
    GPTrainer, PreTrainedGP                                       (per-output ARD GPs, trainer.py)
    SparseGP                                                      (inducing-point GP: every row, m points; sparse.py)
    BatchedSparseGP                                               (up to eight of them served in one call; sparse_batch.py)
    PosteriorPaths, draw_path_randomness                          (posterior function draws, sampled rollouts; paths.py)
    BatchedPosteriorPaths, draw_batch_path_randomness             (the same for the per-axis batch, all models in one call)
    SparsePosteriorPaths, draw_sparse_path_randomness             (the same for SparseGP: paths over the m inducing inputs)
    BatchedSparsePosteriorPaths, draw_sparse_batch_path_randomness  (... and for BatchedSparseGP, all models in one call)
    evaluate_gp, ShardedPredictor, sharded_gram
"""
from .kernels import RBF, ConstantKernel, WhiteKernel  # noqa: F401
from .gpr import GaussianProcessRegressor  # noqa: F401
from .simple_gp import SimpleGPEnhancedMPC, SimpleQuadrotorGP  # noqa: F401
from .package_gp import GaussianProcess  # noqa: F401
from .trainer import GPTrainer, PreTrainedGP  # noqa: F401
from .batched import BatchedARDGP  # noqa: F401
from .sparse import SparseGP  # noqa: F401
from .sparse_batch import BatchedSparseGP  # noqa: F401
from .paths import BatchedPosteriorPaths, PosteriorPaths, draw_batch_path_randomness, draw_path_randomness  # noqa: F401
from .paths import (BatchedSparsePosteriorPaths, SparsePosteriorPaths, draw_sparse_batch_path_randomness,  # noqa: F401
                    draw_sparse_path_randomness)
from .evaluate import evaluate_gp  # noqa: F401
from .sharded import ShardedPredictor, gram_slab_bounds, shard_bounds, sharded_gram, sharded_predict  # noqa: F401

__all__ = ["GaussianProcessRegressor", "RBF", "WhiteKernel", "ConstantKernel", "SimpleQuadrotorGP",
           "SimpleGPEnhancedMPC", "GaussianProcess", "GPTrainer", "PreTrainedGP", "evaluate_gp",
           "ShardedPredictor", "shard_bounds", "sharded_predict", "sharded_gram", "gram_slab_bounds", "BatchedARDGP", "SparseGP",
           "BatchedSparseGP", "PosteriorPaths", "draw_path_randomness", "BatchedPosteriorPaths", "draw_batch_path_randomness",
           "SparsePosteriorPaths", "draw_sparse_path_randomness", "BatchedSparsePosteriorPaths", "draw_sparse_batch_path_randomness"]
