"""MI355X-native batched LDPC belief-propagation decoder behind the ldpc-toolbox decoder
boundary.  The product is libldpc_toolbox.so (HIP kernels + C ABI, see include/ldpc_toolbox.h);
this package is the Python mirror of the reference's interface for that path."""
from . import _capi
from .decoder import (ALL_IMPLEMENTATIONS, CORRECTED_MINSUM_IMPLEMENTATIONS, FAST_IMPLEMENTATIONS, DecoderImplementation, DecoderOutput, DecoderUnavailable, Encoder,
                      I8_IMPLEMENTATIONS, IMPLEMENTATIONS, MINSUM_I8_IMPLEMENTATIONS, LdpcDecoder, Simulator)
from .bch import BchCode
from .demodulator import Demodulator
from .nr_link import NrLink
from .nr_qam import NrQam
from .nr_rate_match import NrRateMatcher
from .nr_transport_block import NrTransportBlock, nr_base_graph
from .sparse import SparseMatrix

code_alist = _capi.code_alist

__all__ = ["ALL_IMPLEMENTATIONS", "BchCode", "CORRECTED_MINSUM_IMPLEMENTATIONS", "FAST_IMPLEMENTATIONS", "I8_IMPLEMENTATIONS", "DecoderImplementation", "DecoderOutput", "DecoderUnavailable", "Demodulator", "Encoder",
           "IMPLEMENTATIONS", "MINSUM_I8_IMPLEMENTATIONS", "LdpcDecoder", "NrLink", "NrQam", "NrRateMatcher", "NrTransportBlock", "Simulator", "SparseMatrix", "code_alist", "nr_base_graph"]
