"""The one list of feature headers (occlusions4d_amd._lib.FEATURE_HEADERS) covers include/: every occ4d*.h but occ4d.h is a row of
it, and the merged table the binding iterates holds every header's symbols once."""
import os

import occlusions4d_amd as pk


def test_registered_headers_are_the_files_of_include():
    lib = pk._lib
    on_disk = {f for f in os.listdir(lib.INCLUDE) if f.startswith('occ4d') and f.endswith('.h')}
    assert on_disk == set(lib.FEATURE_HEADERS.values()) | {'occ4d.h'}
    assert len(set(lib.FEATURE_HEADERS.values())) == len(lib.FEATURE_HEADERS)
    for prefix, name in lib.FEATURE_HEADERS.items():
        assert getattr(lib, prefix + '_HEADER_PATH') == os.path.join(lib.INCLUDE, name)


def test_all_signatures_is_the_sum_of_the_tables():
    lib = pk._lib
    tables = [lib.SIGNATURES] + [getattr(lib, prefix + '_SIGNATURES') for prefix in lib.FEATURE_HEADERS]
    assert len(lib.ALL_SIGNATURES) == sum(len(t) for t in tables)
    for t in tables:
        assert all(lib.ALL_SIGNATURES[name] == sig for name, sig in t.items())
