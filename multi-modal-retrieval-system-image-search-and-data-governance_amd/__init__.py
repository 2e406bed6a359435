"""MI355X-native CLIP encode + cosine top-k, behind the call surface the reference uses.

Public surface (mirrors ``import clip`` as used in reference code/test_clip.py:6-16 and
code/search_image.py:327-338, plus the HF flavour of code/test_taiyi.py:17-30):

    model, preprocess = load("ViT-B/32", device="cuda")
    tokens = tokenize(...)                       # ids pass-through (BPE vocab absent offline)
    model.encode_image(x) / model.encode_text(t) / model(image, text)
    model.get_image_features(pixel_values=x)     # HF spelling
    similarity(features, ref, scale=100.)        # code/search_image.py:107
    cosine_topk(queries, gallery, k)             # code/utils.py:17 generalised
    cosine_topk_deep(queries, gallery, k)        # the same for k up to 4096 (recall@100, np.argsort(d)[:shots])
    cosine_range(queries, gallery, threshold)    # code/search_image.py:58-117 (score >= threshold), exact fp64
    threshold_sweep(queries, gallery, labels, targets, thresholds)   # find_thresholds / evaluate_thresholds: TP, FP per grid point
    cosine_decide(queries, gallery, thresholds)  # code/merge_dataset.py:259-311: a threshold per class, Q exact row masks; en | cn
    cosine_topk(..., row_masks=leave_out_masks(Q, N, qids, rows))   # code/search_image.py:167-182: a gallery per query, one pass
    cosine_assign(gallery, centroids, bias)      # KMeans' assignment step (code/search_image.py:185-292): arg-max over K per row
    kmeans / cluster_sums / reference_vector_by_clustering   # get_cluster_features on the GPU, for a gallery or for shots
    kmeans_plusplus / kmeans(init="k-means++")   # sklearn's default KMeans seeding on the device, exact and reproducible
    silhouette_score / silhouette_samples / select_k         # code/search_image.py:256-259: score each K, one pairwise scan
    outlier_filter / trimmed_centers / rank_in_clusters      # code/search_image.py:295-318: outlier-trimmed class centres, exact
    dedup.near_duplicate_pairs / keep_first      # tool/find_repeated_in_same_folder.py on the GPU gallery
    hash_duplicate_pairs / find_hash_duplicates  # the same tool's own rule: phash / dhash / whash, any distance <= 5
    hash_cross_matches / cross_set_duplicates    # tool/delete repeated.py: dhash of a train image against a test set
    image_hashes / find_image_duplicates         # imagehash's phash / dhash / whash from decoded pixels, Pillow's bytes; hashes_to_hex
    TipAdapterF(keys, values, clip_weights, alpha, beta).fit(...)    # code/main_custom.py:148-247: train the cache keys, AdamW + cosine
    random_resized_crop_params / augment_batch   # code/custom.py:24-29: RandomResizedCrop + flip of decoded images, Pillow's bytes
    build_cache_model_augmented / augmented_features   # code/utils.py:99-132, main_custom.py:166-170 from decoded images
    decode_jpeg / decode_jpeg_batches / jpeg_info   # Image.open(f).convert("RGB") for baseline JPEG files, Pillow's bytes, on the GPU
    encode_jpeg / save_jpeg / encode_jpeg_batches   # img.save(f, 'JPEG', quality=95) from GPU pixels (tool/Image format conversion.py), Pillow's bytes
    GalleryIndex / ShardedGalleryIndex           # row-sharded gallery, RCCL all-gather of top-k

Everything that computes runs in hand-written HIP kernels from ``csrc/libmmr_hip.so``
through the C ABI declared in ``include/mmr.h``; there is no CPU fallback.
"""
from .config import MODEL_CONFIGS, ClipConfig, TowerConfig, available_models, get_config  # noqa: F401

__all__ = [
    "available_models", "get_config", "load", "tokenize", "similarity", "cosine_topk", "l2_normalize",
    "GalleryIndex", "ShardedGalleryIndex", "CLIP", "cosine_range", "gallery_self_join", "dedup",
    "threshold_sweep", "ThresholdSweep", "cosine_topk_deep",
    "cosine_decide", "DecisionMasks", "leave_out_masks",
    "cosine_assign", "cluster", "cluster_sums", "kmeans", "KMeansResult", "reference_vector_by_clustering",
    "kmeans_plusplus", "kmeanspp_trials", "kmeanspp_variates",
    "silhouette_sums", "silhouette_samples", "silhouette_score", "select_k", "SelectKResult",
    "rank_in_clusters", "ClusterRanking", "percentile_trim", "trimmed_centers", "TrimmedCenters", "outlier_filter",
    "hashes_from_hex", "hash_duplicate_pairs", "find_hash_duplicates", "hash_cross_matches", "cross_set_duplicates",
    "image_hashes", "hashes_to_hex", "find_image_duplicates", "ImageHashPlan",
    "TipAdapterF", "cosine_lr", "tip_adapter_grid", "TipGrid", "search_hp",
    "random_resized_crop_params", "augment_batch", "build_cache_model_augmented", "augmented_features",
    "decode_jpeg", "decode_jpeg_batches", "jpeg_info", "JpegPlan",
    "encode_jpeg", "save_jpeg", "encode_jpeg_batches", "JpegEncodePlan", "jpeg_quant_tables",
]

_LAZY = {
    "load": "clip", "tokenize": "clip", "CLIP": "clip",
    "similarity": "search", "cosine_topk": "search", "cosine_topk_deep": "search", "cosine_range": "search", "threshold_sweep": "search", "ThresholdSweep": "search", "cosine_decide": "search", "DecisionMasks": "search", "leave_out_masks": "search", "gallery_self_join": "search", "l2_normalize": "search",
    "GalleryIndex": "search", "ShardedGalleryIndex": "search", "merge_topk": "search",
    "cosine_assign": "search", "cluster_sums": "cluster", "kmeans": "cluster", "KMeansResult": "cluster",
    "reference_vector_by_clustering": "cluster",
    "kmeans_plusplus": "cluster", "kmeanspp_trials": "cluster", "kmeanspp_variates": "cluster",
    "silhouette_sums": "cluster", "silhouette_samples": "cluster", "silhouette_score": "cluster", "select_k": "cluster",
    "SelectKResult": "cluster",
    "rank_in_clusters": "cluster", "ClusterRanking": "cluster", "percentile_trim": "cluster", "trimmed_centers": "cluster",
    "TrimmedCenters": "cluster", "outlier_filter": "cluster",
    "hashes_from_hex": "dedup", "hash_duplicate_pairs": "dedup", "find_hash_duplicates": "dedup",
    "hash_cross_matches": "dedup", "cross_set_duplicates": "dedup",
    "image_hashes": "dedup", "hashes_to_hex": "dedup", "find_image_duplicates": "dedup", "ImageHashPlan": "dedup",
    "TipAdapterF": "tip_adapter", "cosine_lr": "tip_adapter",
    "tip_adapter_grid": "tip_adapter", "TipGrid": "tip_adapter", "search_hp": "tip_adapter",
    "random_resized_crop_params": "preprocess", "augment_batch": "preprocess",
    "build_cache_model_augmented": "gallery", "augmented_features": "gallery",
    "decode_jpeg": "jpeg", "decode_jpeg_batches": "jpeg", "jpeg_info": "jpeg", "JpegPlan": "jpeg",
    "encode_jpeg": "jpeg", "save_jpeg": "jpeg", "encode_jpeg_batches": "jpeg", "JpegEncodePlan": "jpeg", "jpeg_quant_tables": "jpeg",
    "tip_adapter_logits": "search", "load_text_encoder": "bert", "BertTextEncoder": "bert", "encode_gallery": "gallery", "build_cache": "gallery",
}


def __getattr__(name):
    # Lazy so that config/weights/synth import on a CPU-only box without touching the GPU lib.
    if name in _LAZY:
        import importlib

        mod = importlib.import_module(f"{__name__}.{_LAZY[name]}")
        return getattr(mod, name)
    if name in ("synth", "weights", "search", "clip", "config", "_lib", "gallery", "preprocess", "bert", "tokenizer", "checkpoint", "dedup", "cluster", "tip_adapter", "jpeg"):
        import importlib

        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(name)
