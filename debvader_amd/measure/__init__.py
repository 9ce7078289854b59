"""Catalogue measurement of deblended galaxies (the reference's debvader.measure package is empty)."""
