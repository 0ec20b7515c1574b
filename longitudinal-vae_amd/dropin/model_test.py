"""model_test.py surface (reference model_test.py:11-143) backed by lvae_amd (HIP): the exact-GP test-set
evaluation of models trained with the exact KL and its GP-approximation counterpart."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lvae_amd.evaluation import MSE_test, MSE_test_GPapprox, VAEtest, predict_gp  # noqa: E402,F401

__all__ = ["predict_gp", "MSE_test", "MSE_test_GPapprox", "VAEtest"]
