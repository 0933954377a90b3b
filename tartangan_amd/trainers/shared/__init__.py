"""Trainers of the shared-filter model family (reference trainers/shared)."""
