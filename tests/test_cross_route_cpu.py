"""CrossRoute's arithmetic — the ``kv_tiled`` selector, the ``max_group`` bound or its refusal, the image blocks with their row
slices and the ``kv_len`` slice of every launch — against a literal table.

The table was produced from the four helpers CrossRoute replaced (BertModel._cross_tiled / _cross_bound / _cross_blocks /
_cross_len_arg, called unbound on a stub with LONG_KEYS = 768 and MAX_IMAGES_PER_LAUNCH = 2; the row slice of a block as
run_layers computed it) at the commit before the route existed, over
  Te in {768, 769} x tiled in {False, True} x unit form x Nq in {1, 3, 33} x B in {2, 5}
with the unit forms: uniform grouping (group 1 and 3), ``index``, and ``groups`` with max_group 0, 3 and 40.  Query batches:
B * group for uniform grouping, 3 B for the other two.  Nothing here touches a device."""
import types

import pytest
import torch

from vidil_amd import kernels as K
from vidil_amd.med import CrossKV, CrossRoute

MODEL = types.SimpleNamespace(LONG_KEYS=768, MAX_IMAGES_PER_LAUNCH=2)

# (Te, tiled, form, group, max_group, Nq, B) -> kv_tiled, bound | refusal text, [(b0, b1, r0, r1, (kv_len offset, numel))]
TABLE = [
    (768, False, 'uniform', 1, 0, 1, 2, False, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, False, 'uniform', 1, 0, 1, 5, False, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, False, 'uniform', 1, 0, 3, 2, False, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, False, 'uniform', 1, 0, 3, 5, False, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, False, 'uniform', 1, 0, 33, 2, False, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, False, 'uniform', 1, 0, 33, 5, False, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, False, 'uniform', 3, 0, 1, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'uniform', 3, 0, 1, 5, False, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, False, 'uniform', 3, 0, 3, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'uniform', 3, 0, 3, 5, False, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, False, 'uniform', 3, 0, 33, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'uniform', 3, 0, 33, 5, False, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, False, 'index', 1, 0, 1, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'index', 1, 0, 1, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'index', 1, 0, 3, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'index', 1, 0, 3, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'index', 1, 0, 33, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'index', 1, 0, 33, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 0, 1, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 0, 1, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 0, 3, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 0, 3, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 0, 33, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 0, 33, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 3, 1, 2, False, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 3, 1, 5, False, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 3, 3, 2, False, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 3, 3, 5, False, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 3, 33, 2, False, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 3, 33, 5, False, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 40, 1, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 40, 1, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 40, 3, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 40, 3, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (768, False, 'groups', 1, 40, 33, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, False, 'groups', 1, 40, 33, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'uniform', 1, 0, 1, 2, True, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, True, 'uniform', 1, 0, 1, 5, True, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, True, 'uniform', 1, 0, 3, 2, True, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, True, 'uniform', 1, 0, 3, 5, True, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, True, 'uniform', 1, 0, 33, 2, True, 0, [(0, 2, 0, 2, (0, 2))]),
    (768, True, 'uniform', 1, 0, 33, 5, True, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (768, True, 'uniform', 3, 0, 1, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'uniform', 3, 0, 1, 5, True, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, True, 'uniform', 3, 0, 3, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'uniform', 3, 0, 3, 5, True, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, True, 'uniform', 3, 0, 33, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'uniform', 3, 0, 33, 5, True, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (768, True, 'index', 1, 0, 1, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'index', 1, 0, 1, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'index', 1, 0, 3, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'index', 1, 0, 3, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'index', 1, 0, 33, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'index', 1, 0, 33, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 0, 1, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 0, 1, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 0, 3, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 0, 3, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 0, 33, 2, True, 0, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 0, 33, 5, True, 0, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 3, 1, 2, True, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 3, 1, 5, True, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 3, 3, 2, True, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 3, 3, 5, True, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 3, 33, 2, True, 3, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 3, 33, 5, True, 3, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 40, 1, 2, True, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 40, 1, 5, True, 40, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 40, 3, 2, True, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 40, 3, 5, True, 40, [(0, 5, 0, 15, (0, 15))]),
    (768, True, 'groups', 1, 40, 33, 2, True, 40, [(0, 2, 0, 6, (0, 6))]),
    (768, True, 'groups', 1, 40, 33, 5, True, 40, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'uniform', 1, 0, 1, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 1): order the pairs image-major and use group_start', [(0, 2, 0, 2, (0, 2))]),
    (769, False, 'uniform', 1, 0, 1, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 1): order the pairs image-major and use group_start', [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, False, 'uniform', 1, 0, 3, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 2, 0, 2, (0, 2))]),
    (769, False, 'uniform', 1, 0, 3, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, False, 'uniform', 1, 0, 33, 2, False, 0, [(0, 2, 0, 2, (0, 2))]),
    (769, False, 'uniform', 1, 0, 33, 5, False, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, False, 'uniform', 3, 0, 1, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'uniform', 3, 0, 1, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, False, 'uniform', 3, 0, 3, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 9): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'uniform', 3, 0, 3, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 9): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, False, 'uniform', 3, 0, 33, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'uniform', 3, 0, 33, 5, False, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, False, 'index', 1, 0, 1, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 1): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'index', 1, 0, 1, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 1): order the pairs image-major and use group_start', [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'index', 1, 0, 3, 2, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'index', 1, 0, 3, 5, False, 'cross-attention over 769 > 768 encoder states needs more than 32 query rows per unit (got 3): order the pairs image-major and use group_start', [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'index', 1, 0, 33, 2, False, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'index', 1, 0, 33, 5, False, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 0, 1, 2, False, 33, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 0, 1, 5, False, 33, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 0, 3, 2, False, 11, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 0, 3, 5, False, 11, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 0, 33, 2, False, 1, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 0, 33, 5, False, 1, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 3, 1, 2, False, 33, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 3, 1, 5, False, 33, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 3, 3, 2, False, 11, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 3, 3, 5, False, 11, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 3, 33, 2, False, 3, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 3, 33, 5, False, 3, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 40, 1, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 40, 1, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 40, 3, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 40, 3, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (769, False, 'groups', 1, 40, 33, 2, False, 40, [(0, 2, 0, 6, (0, 6))]),
    (769, False, 'groups', 1, 40, 33, 5, False, 40, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'uniform', 1, 0, 1, 2, 2, 0, [(0, 2, 0, 2, (0, 2))]),
    (769, True, 'uniform', 1, 0, 1, 5, 2, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, True, 'uniform', 1, 0, 3, 2, 2, 0, [(0, 2, 0, 2, (0, 2))]),
    (769, True, 'uniform', 1, 0, 3, 5, 2, 0, [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, True, 'uniform', 1, 0, 33, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 33): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 2, (0, 2))]),
    (769, True, 'uniform', 1, 0, 33, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 33): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 2, (0, 2)), (2, 4, 2, 4, (2, 2)), (4, 5, 4, 5, (4, 1))]),
    (769, True, 'uniform', 3, 0, 1, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'uniform', 3, 0, 1, 5, 2, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, True, 'uniform', 3, 0, 3, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'uniform', 3, 0, 3, 5, 2, 0, [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, True, 'uniform', 3, 0, 33, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 99): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'uniform', 3, 0, 33, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 99): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6)), (2, 4, 6, 12, (6, 6)), (4, 5, 12, 15, (12, 3))]),
    (769, True, 'index', 1, 0, 1, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'index', 1, 0, 1, 5, 2, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'index', 1, 0, 3, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'index', 1, 0, 3, 5, 2, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'index', 1, 0, 33, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 33): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'index', 1, 0, 33, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 33): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 0, 1, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 0, 1, 5, 2, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 0, 3, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 0, 3, 5, 2, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 0, 33, 2, 2, 0, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 0, 33, 5, 2, 0, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 3, 1, 2, 2, 3, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 3, 1, 5, 2, 3, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 3, 3, 2, 2, 3, [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 3, 3, 5, 2, 3, [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 3, 33, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 99): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 3, 33, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 99): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 40, 1, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 40): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 40, 1, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 40): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 40, 3, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 120): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 40, 3, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 120): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 5, 0, 15, (0, 15))]),
    (769, True, 'groups', 1, 40, 33, 2, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 1320): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 2, 0, 6, (0, 6))]),
    (769, True, 'groups', 1, 40, 33, 5, 2, 'cross-attention over 769 > 768 encoder states in fragment tiles serves at most 32 query rows per unit (got 1320): build the session with tiled_cross=False, whose launches go to the long-key form', [(0, 5, 0, 15, (0, 15))]),
]


def _route(Te, tiled, form, group, max_group, B, with_len):
    rows = B * group if form == "uniform" else 3 * B
    return CrossRoute(MODEL, CrossKV(None, None, B, Te, 0, tiled=tiled), rows,
                      index=torch.zeros(rows, dtype=torch.int32) if form == "index" else None, group=group,
                      groups=torch.zeros(B + 1, dtype=torch.int32) if form == "groups" else None, max_group=max_group,
                      kv_len=torch.ones(rows, dtype=torch.int32) if with_len else None)


def test_the_table_covers_the_grid():
    keys = [r[:7] for r in TABLE]
    assert len(set(keys)) == len(keys) == 2 * 2 * 6 * 3 * 2
    assert {r[0] for r in TABLE} == {768, 769} and {r[5] for r in TABLE} == {1, 3, 33} and {r[6] for r in TABLE} == {2, 5}


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "-".join(str(x) for x in r[:7]))
def test_route_equals_the_helpers_it_replaced(row):
    Te, tiled, form, group, max_group, Nq, B, kv_tiled, bound, blocks = row
    route = _route(Te, tiled, form, group, max_group, B, True)
    assert route.tiled == kv_tiled and type(route.tiled) is type(kv_tiled)
    if isinstance(bound, str):
        with pytest.raises(K.VidilHipError) as e:
            route.bound(Nq)
        assert str(e.value) == bound
    else:
        assert route.bound(Nq) == bound
    assert route.blocks() == [b[:4] for b in blocks]
    bare = _route(Te, tiled, form, group, max_group, B, False)
    for b0, b1, r0, r1, (off, n) in blocks:
        arg = route.len_arg(r0, r1)
        assert list(arg) == ["kv_len"] and (arg["kv_len"].storage_offset(), arg["kv_len"].numel()) == (off, n)
        assert arg["kv_len"].untyped_storage().data_ptr() == route.kv_len.untyped_storage().data_ptr()
        assert bare.len_arg(r0, r1) == {}


def test_kv_len_refusal_keeps_its_text():
    for bad in (torch.ones(3, dtype=torch.int64), torch.ones(4, dtype=torch.int32), torch.ones(6, dtype=torch.int32)[::2]):
        with pytest.raises(K.VidilHipError) as e:
            CrossRoute(MODEL, CrossKV(None, None, 3, 10, 0), 3, kv_len=bad)
        assert str(e.value) == (f"run_layers: cross_kv_len must be a contiguous i32 [3] tensor (one length per query batch), got "
                                f"{bad.dtype} {tuple(bad.shape)}")
