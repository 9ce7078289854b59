"""Source detection (reference: src/debvader/detect/)."""
