"""Evaluation of trained models (the reference's cpc/eval): ABX phone discriminability on the MI355X kernels."""
