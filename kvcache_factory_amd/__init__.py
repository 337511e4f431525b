"""MI355X-native KV-cache compression hot path (drop-in for KVCache-Factory's update_kv path).

Public surface mirrors the reference (assassin808/KVCache-Factory @ 2025-02-18):
    kvcache_factory_amd.monkeypatch.replace_llama / replace_mistral      (pyramidkv/monkeypatch.py:19,92)
    kvcache_factory_amd.pyramidkv_utils.{SnapKV,PyramidKV,H2OKV,StreamingLLMKV}Cluster.update_kv
                                                                         (pyramidkv/pyramidkv_utils.py:197,306,533,595)
    kvcache_factory_amd.pyramidkv_utils.init_{pyramidkv,snapkv,H2O,StreamingLLM}   (:880-1031)
All compute runs in hand-written HIP kernels (csrc/, libkvc_hip.so) through the C-ABI of include/kvc.h;
there is no CPU or eager-PyTorch fallback: if the extension is missing the import of `_kvc` raises.
"""
__version__ = "0.1.0"
__all__ = ["QuantizedCompressedCache", "QuantizedCompressedLayer", "KVQuantCompressedCache", "KVQuantCompressedLayer",
           "DecodeCompressedCache", "DecodeCompressedLayer", "HeavyHitterCache", "HeavyHitterLayer", "GraphDecoder",
           "BoundedDeviceLayer", "BoundedHeavyHitterLayer", "QuantizedDeviceLayer"]


def __getattr__(name):
    # the quantized, decode-compressed and heavy-hitter caches (cache.py) are exported lazily: importing the package does not
    # import transformers
    if name == "GraphDecoder":                                # graph-replayed decoding (graph_decode.py)
        from .graph_decode import GraphDecoder
        return GraphDecoder
    if name in __all__:
        from . import cache
        return getattr(cache, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
