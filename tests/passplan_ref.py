"""Which launches a pass runs, restated in numpy from the host code as it stood before csrc/rope_passplan.h existed: every function
below is one function (or one stretch of enqueue_eval) of that rope_abi.hip, over arrays of passes instead of a context, with the
C arithmetic kept (all operands are non-negative, so // is C's division).  tests/test_passplan_host.py holds plan_pass() to it."""
import numpy as np

# rope_set_strategy's bits and the loss codes (include/rope_s3d.h)
NO_LAYERS, NO_SPLIT, NO_PARENTS, NO_QUEUE, CLIP_KERNELS, SEPARATE_GEOMETRY, NO_GEOMETRY_CACHE, NO_KEPT_FRAGMENTS = (1 << i for i in range(8))
LOSS_DEPTH, LOSS_FULL, LOSS_LOOKUP, LOSS_TSWEEP, LOSS_CAMFULL = range(5)
EVAL_SINGLE, EVAL_TARGETS, EVAL_VIEWS = range(3)
SCORE_GTILE, SCORE_QUEUE, SCORE_PLAIN = range(3)

INPUTS = ('C', 'n_tiles', 'n_layers', 'n_parents', 'n_render', 'loss', 'kind', 'frame_index', 'strategy', 'n_cu', 'q_weighted', 'clip', 'skip',
          'split_target', 'split_min', 'split_min_many', 'split_cap', 'score_target', 'geo_rows', 'layer_min_wg')
OUTPUTS = ('layers', 'n_shared', 'parents', 'lo_first', 'layer_queue', 'weighted', 'split', 'own_geometry', 'fused_geometry', 'scoring', 'slices',
           'cache_scope', 'cacheable', 'fragment_scope', 'clip')
# rope_ctx's members as they were initialised, n_cu as rope_create falls back to it; a pass of rope_eval_resident on six links
DEFAULTS = dict(C=1, n_tiles=4, n_layers=1, n_parents=1, n_render=6, loss=LOSS_DEPTH, kind=EVAL_SINGLE, frame_index=0, strategy=0, n_cu=256,
                q_weighted=1, clip=0, skip=0, split_target=512, split_min=8, split_min_many=3, split_cap=64, score_target=6144, geo_rows=48,
                layer_min_wg=64)


def _busy_tiles(n_tiles):
    """written out in layers_pay, queue_weights and enqueue_eval: std::max(std::min(2, n_tiles), n_tiles / 3)"""
    return np.maximum(np.minimum(2, n_tiles), n_tiles // 3)


def want_layers(r):
    return r['n_layers'] * 4 <= r['C']


def layers_pay(r):
    return (r['C'] > 256) | (r['n_layers'] * _busy_tiles(r['n_tiles']) >= r['layer_min_wg'])


def want_parents(r):
    return r['n_parents'] * 4 <= r['n_layers']


def queue_weights(r):
    """non-null"""
    return (r['q_weighted'] != 0) & (r['C'] > 256) & (r['C'] * _busy_tiles(r['n_tiles']) <= 256 * 2 * r['n_cu'])


def use_parents(r, n_shared):
    no = (n_shared != 3) | ~want_parents(r) | ((r['strategy'] & NO_PARENTS) != 0)
    return ~no & ~(queue_weights(r) & ((r['strategy'] & NO_QUEUE) == 0))


def enqueue_layers(r):
    """-> whether the layers go through launch_layer_queue"""
    return queue_weights(r) & ((r['strategy'] & NO_QUEUE) == 0)


def enqueue_geometry(r, n_shared):
    """-> (the fused launch_fk_bounds, lo_first of launch_bounds)"""
    return r['C'] <= 256, np.where(use_parents(r, n_shared), 2, 0)


def geometry_key(r, n_shared):
    """-> the key's parents, weighted (queue is a bit of `strategy`, which the key holds as well); clip is use_clip's verdict"""
    return use_parents(r, n_shared), queue_weights(r)


def enqueue_eval(rows):
    """rows: (n, len(INPUTS)) integers -> (n, len(OUTPUTS)) integers, what enqueue_eval and the functions it called decided"""
    rows = np.asarray(rows, np.int64)
    r = {k: rows[:, i] for i, k in enumerate(INPUTS)}
    C, n_tiles, strategy = r['C'], r['n_tiles'], r['strategy']
    off = lambda bit: (strategy & bit) == 0                                                   # noqa: E731
    views = r['kind'] == EVAL_VIEWS
    layers = ~views & want_layers(r) & layers_pay(r) & off(NO_LAYERS)
    n_shared = np.where(layers, np.minimum(3, r['n_render']), 0)
    in_scope = (r['kind'] == EVAL_SINGLE) & layers & (C > 256) & (r['frame_index'] == 0)
    cacheable = in_scope & off(NO_GEOMETRY_CACHE) & (r['skip'] == 0)
    # frag_scope = hit && ...: a hit is a cacheable pass whose key the context holds
    frag_scope = cacheable & (r['loss'] != LOSS_CAMFULL) & off(NO_KEPT_FRAGMENTS | NO_QUEUE)
    pairs = C * _busy_tiles(n_tiles)
    floor_ = np.where(pairs <= 256, r['split_min'], r['split_min_many'])
    split = np.maximum(np.minimum(r['split_cap'], r['split_target'] // np.maximum(1, pairs)), np.minimum(floor_, r['split_cap']))
    split = np.where((split < 2) | (pairs > 4 * r['split_target']), 1, split)
    split = np.where(~layers & off(NO_SPLIT), split, 1)
    geo = (split > 1) & ~views & (C <= r['geo_rows']) & (n_tiles <= 4) & off(SEPARATE_GEOMETRY)
    slices = np.ones_like(C)
    for _ in range(3):                                                                        # while (slices < 8 && ...) slices *= 2
        slices = np.where((slices < 8) & (C * n_tiles * slices * 2 <= r['score_target']), slices * 2, slices)
    slices = np.where(split > 1, slices, 1)
    scoring = np.where(split > 1, SCORE_GTILE, np.where((C > 256) & off(NO_QUEUE), SCORE_QUEUE, SCORE_PLAIN))
    fused, lo_first = enqueue_geometry(r, n_shared)
    parents, weighted = geometry_key(r, n_shared)
    out = dict(layers=layers, n_shared=n_shared, parents=parents, lo_first=lo_first, layer_queue=enqueue_layers(r), weighted=weighted, split=split,
               own_geometry=geo, fused_geometry=fused, scoring=scoring, slices=slices, cache_scope=in_scope, cacheable=cacheable,
               fragment_scope=frag_scope, clip=r['clip'] != 0)
    return np.stack([np.asarray(out[k]).astype(np.int64) for k in OUTPUTS], axis=1)
