"""clonos_amd -- MI355X-native causal-log engine for Clonos (decode, delta-slice, truncate,
replay-prep on gfx950).  The compute path is libclonos_engine.so (HIP); this package is
the host-side mirror of the reference Java interfaces."""
from . import determinants
from ._lib import ClonosError
from .engine import (DIFF, DIGEST, CausalLogID, DecodedBatch, DecodedColumns, Engine, ThreadCausalLog, columnize_host, gather_payloads_host,
                     digest_host, digest_prefixes_host, encode_columns_host, lcp_host, PackedColumns, pack_columns_host,
                     unpack_columns_host, unpack_packed_host, PackedWide, pack_wide_host, unpack_wide_host,
                     encode_columns_packed_wide_host, PackedPayloads, pack_payloads_host, unpack_payloads_host)

__all__ = ["Engine", "ThreadCausalLog", "CausalLogID", "DecodedBatch", "ClonosError", "determinants", "DIGEST",
           "digest_host", "DIFF", "lcp_host", "digest_prefixes_host", "DecodedColumns", "columnize_host", "gather_payloads_host",
           "encode_columns_host", "PackedColumns", "pack_columns_host", "unpack_columns_host",
           "unpack_packed_host", "PackedWide", "pack_wide_host", "unpack_wide_host",
           "encode_columns_packed_wide_host", "PackedPayloads", "pack_payloads_host", "unpack_payloads_host"]
