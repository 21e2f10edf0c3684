"""recommender_amd — MI355X-native (gfx950) sparse-embedding and feature-interaction engine.

Hot path in hand-written HIP behind the C-ABI of include/recsys_hip.h (librecsys_hip.so);
host side mirrors the reference's Keras layer/model call surfaces (neoyinyao/Recommender).
"""
from . import _lib  # noqa: F401

__version__ = "0.1.0"

_TABLES = ("Embedding", "EmbeddingBag", "SlabEmbedding")
_QUANTIZED = ("QuantizedEmbedding", "QuantizedEmbeddingBag", "from_float", "quantize_embeddings")


def __getattr__(name):
    # the table classes, importable from the package (resolved on first use)
    if name in _TABLES:
        from . import embedding
        return getattr(embedding, name)
    if name in _QUANTIZED:
        from . import quantized
        return getattr(quantized, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
