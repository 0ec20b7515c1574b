"""validation.py surface (reference validation.py:8-175) backed by lvae_amd (HIP): the validation-set loss of
the GP-approximation regimes and the all-dims DUBO."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from lvae_amd.validation import validate, validation_dubo  # noqa: E402,F401

__all__ = ["validate", "validation_dubo"]
