"""Iterative deblending of a field (reference: src/debvader/deblend_iterative/)."""
