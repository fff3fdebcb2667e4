"""Mirrors of the reference's ``src/utilities`` scripts."""
