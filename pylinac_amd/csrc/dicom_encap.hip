// Encapsulated Pixel Data that is already ON the device (the members of a ZIP archive after pl_zip_extract): the two steps
// dicom.load_zip(encapsulated=True) puts between the extraction and the RLE Lossless / JPEG Lossless decoders.
//
// enc_index_kernel (pl_dicom_encap_index): the item walk of PS3.5 section A.4 -- the Basic Offset Table item, one item per
//   fragment, the Sequence Delimitation Item -- for M values side by side, ONE wave per value.  The walk is a chain of
//   dependent reads: lane 0 takes the 8 bytes of an item header (byte loads, an item may start at any address), the wave
//   keeps tag, length and position in scalar registers (readfirstlane) and all 64 lanes copy the head of the fragment --
//   its first min(length, head_bytes) bytes, zeros behind them -- into the result block, four bytes a lane and pass.  The
//   host parses RLE segment headers and JPEG markers from those heads; the payloads stay where they are.
//   Every read lies inside the member's window [first, end), which is checked against the buffer before anything is read;
//   a length is compared with what is LEFT of the window (64-bit differences, never a sum with an untrusted length) before
//   the walk hops over it.  Every store lies inside the member's slots: nothing is written for a fragment at or beyond
//   `cap` or a table entry at or beyond `tcap`, they are only counted.
//
// enc_copy_kernel (pl_copy_ranges): R byte ranges from one device buffer into another, any alignment on either side -- what
//   lays the fragments of a frame that spans several end to end.  Built like dicom_decode_kernel's loads: the destination is
//   written in 16-byte stores on 16-byte boundaries, each fed by a 4-dword load on a DWORD boundary (the source's address
//   rounded down to 4 bytes, not to 16) plus the dword that follows, funnel-shifted by the source's misalignment against it
//   (v_alignbit); up to 15 bytes in front of the first and behind the last aligned block are copied byte by byte, so no byte
//   outside a destination range is written.  Traffic: 2 x the bytes; its rate out of HBM has not been measured.
//
// A translation unit of its own in the library.  The CPU emulator of the tests builds a fixed list of files, dicom.hip among
// them: there dicom.hip includes this file after pl_common.h (PL_ENCAP_IN_DICOM), which is why nothing here may collide with
// dicom.hip's or jpeg_lossless.hip's names.
#ifndef PL_ENCAP_IN_DICOM
#include "pl_common.h"
#endif

namespace {

constexpr int kEncThreads = 256;                            // the copy's workgroup
constexpr int kEncMaxGridY = 65535;

struct alignas(4) EncU4 { unsigned x, y, z, w; };

// where the parts of the result block lie (all sizes are multiples of 8; head_bytes is a multiple of 16)
struct EncLayout {
  int64_t frags, heads, table, info, total;
};
__host__ __device__ inline EncLayout enc_layout(int64_t m, int64_t cap, int64_t tcap, int64_t head_bytes) {
  EncLayout l;
  l.frags = 0;
  l.heads = l.frags + m * cap * 24;
  l.info = l.heads + m * cap * head_bytes;
  l.table = l.info + m * 16;
  l.total = (l.table + m * tcap * 4 + 15) & ~(int64_t)15;
  return l;
}

__device__ __forceinline__ unsigned enc_le32(const unsigned char* p) {
  return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24);
}

__global__ void __launch_bounds__(PL_WAVE)
enc_index_kernel(const unsigned char* __restrict__ bytes, int64_t nbytes, const int64_t* __restrict__ first,
                 const int64_t* __restrict__ end, int64_t n_members, int cap, int tcap, int head_bytes,
                 unsigned char* __restrict__ result) {
  const int lane = threadIdx.x;
  const int64_t m = blockIdx.x;
  const EncLayout lay = enc_layout(n_members, cap, tcap, head_bytes);
  int64_t* frags = reinterpret_cast<int64_t*>(result + lay.frags) + m * cap * 3;
  unsigned* heads = reinterpret_cast<unsigned*>(result + lay.heads + m * cap * (int64_t)head_bytes);
  unsigned* table = reinterpret_cast<unsigned*>(result + lay.table) + m * tcap;
  int32_t* info = reinterpret_cast<int32_t*>(result + lay.info) + m * 4;
  const int64_t lo = first[m], hi = end[m];
  if (lo < 0 || hi < lo || hi > nbytes) {                   // nothing is read, nothing but the status is stored
    if (lane == 0) info[0] = PL_ENCAP_DESCRIPTOR;
    return;
  }
  int64_t pos = lo;
  int status = 0, n_frag = 0, n_table = -1;                 // n_table < 0: the table item has not been met
  while (true) {
    if (hi - pos < 8) {
      status |= PL_ENCAP_MALFORMED | PL_ENCAP_NO_DELIMITER;
      break;
    }
    unsigned t = 0, l = 0;
    if (lane == 0) t = enc_le32(bytes + pos), l = enc_le32(bytes + pos + 4);
    const unsigned tag = __builtin_amdgcn_readfirstlane(t), len = __builtin_amdgcn_readfirstlane(l);
    if (tag == 0xE0DDFFFEu) break;
    if (tag != 0xE000FFFEu || len == 0xFFFFFFFFu || (int64_t)len > hi - pos - 8) {
      status |= PL_ENCAP_MALFORMED;
      break;
    }
    const unsigned char* payload = bytes + pos + 8;
    if (n_table < 0) {
      if (len & 3u) {
        status |= PL_ENCAP_TABLE | PL_ENCAP_TABLE_LENGTH;
        break;
      }
      n_table = (int)(len >> 2);
      const int take = n_table < tcap ? n_table : tcap;
      for (int i = lane; i < take; i += PL_WAVE) table[i] = enc_le32(payload + 4 * i);
    } else {
      if (n_frag < cap) {
        if (lane == 0) {
          int64_t* f = frags + (int64_t)n_frag * 3;
          f[0] = pos + 8, f[1] = (int64_t)len, f[2] = pos;
        }
        const int have = len < (unsigned)head_bytes ? (int)len : head_bytes;
        unsigned* head = heads + (int64_t)n_frag * (head_bytes >> 2);
        for (int at = lane * 4; at < head_bytes; at += PL_WAVE * 4) {
          unsigned w = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b)
            if (at + b < have) w |= (unsigned)payload[at + b] << (8 * b);
          head[at >> 2] = w;
        }
      }
      ++n_frag;
    }
    pos += 8 + (int64_t)len;
  }
  if (n_table < 0 && !status) status |= PL_ENCAP_TABLE;     // the delimiter came first: no table item
  if (n_frag > cap || n_table > tcap) status |= PL_ENCAP_CAPACITY;
  if (lane == 0) info[0] = status, info[1] = n_frag, info[2] = n_table < 0 ? 0 : n_table, info[3] = 0;
}

__global__ void __launch_bounds__(kEncThreads)
enc_copy_kernel(const unsigned char* __restrict__ src, int64_t src_bytes, unsigned char* __restrict__ dst, int64_t dst_bytes,
                const int64_t* __restrict__ src_off, const int64_t* __restrict__ len, const int64_t* __restrict__ dst_off,
                int64_t n_ranges, int32_t* __restrict__ status) {
  for (int64_t r = blockIdx.y; r < n_ranges; r += gridDim.y) {
    const int64_t s = src_off[r], n = len[r], d = dst_off[r];
    // (differences of lengths, never sums of an offset and a length: nothing here can overflow)
    const bool inside = s >= 0 && n >= 0 && d >= 0 && s <= src_bytes && n <= src_bytes - s && d <= dst_bytes && n <= dst_bytes - d;
    if (blockIdx.x == 0 && threadIdx.x == 0) status[r] = inside ? 0 : 1;
    if (!inside) continue;
    const unsigned char* from = src + s;
    unsigned char* to = dst + d;
    int64_t front = (int64_t)((16u - (unsigned)((uintptr_t)to & 15u)) & 15u);      // bytes before the first aligned block
    if (front > n) front = n;
    const int64_t nvec = (n - front) >> 4;
    const int64_t back = front + 16 * nvec;                 // the bytes from here on follow the last aligned block
    if (nvec > 0) {
      const unsigned char* body = from + front;
      const unsigned sh = (unsigned)((uintptr_t)body & 3u) * 8u;
      const unsigned* base = reinterpret_cast<const unsigned*>(body - (sh >> 3));
      // a dword that ends beyond the source buffer is put together from the bytes that exist (src is on a 4-byte boundary)
      const unsigned char* whole = src + (src_bytes & ~(int64_t)3);
      EncU4* out = reinterpret_cast<EncU4*>(to + front);
      for (int64_t v = (int64_t)blockIdx.x * kEncThreads + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * kEncThreads) {
        const EncU4 q = *reinterpret_cast<const EncU4*>(base + 4 * v);
        unsigned w[4] = {q.x, q.y, q.z, q.w};
        if (sh) {                                           // (wave-uniform: a property of the range)
          const unsigned char* ep = reinterpret_cast<const unsigned char*>(base + 4 * v + 4);
          unsigned e;
          if (ep + 4 <= whole) {
            e = *reinterpret_cast<const unsigned*>(ep);
          } else {                                          // only its first sh / 8 bytes are used, and those lie in the range
            e = 0;
            for (unsigned b = 0; b < (sh >> 3); ++b) e |= (unsigned)ep[b] << (8 * b);
          }
          w[0] = __builtin_amdgcn_alignbit(w[1], w[0], sh);
          w[1] = __builtin_amdgcn_alignbit(w[2], w[1], sh);
          w[2] = __builtin_amdgcn_alignbit(w[3], w[2], sh);
          w[3] = __builtin_amdgcn_alignbit(e, w[3], sh);
        }
        out[v] = EncU4{w[0], w[1], w[2], w[3]};
      }
    }
    if (blockIdx.x == 0) {                                  // fewer than 16 bytes on either side: one byte a lane
      const int64_t edge = front + (n - back);
      for (int64_t i = threadIdx.x; i < edge; i += kEncThreads) {
        const int64_t at = i < front ? i : back + (i - front);
        to[at] = from[at];
      }
    }
  }
}

}  // namespace

extern "C" int64_t pl_dicom_encap_index_bytes(int64_t n_members, int cap, int tcap, int head_bytes) {
  if (n_members < 1 || n_members > 0x7fffffff || cap < 1 || tcap < 1 || cap > (1 << 24) || tcap > (1 << 24)) return -1;
  if (head_bytes < 16 || head_bytes > PL_DICOM_ENCAP_MAX_HEAD || head_bytes % 16) return -1;
  return enc_layout(n_members, cap, tcap, head_bytes).total;
}

extern "C" int pl_dicom_encap_index(const unsigned char* d_bytes, int64_t nbytes, const int64_t* d_first, const int64_t* d_end,
                                    int64_t n_members, int cap, int tcap, int head_bytes, unsigned char* d_result,
                                    void* stream) {
  PL_REQUIRE(d_bytes && d_first && d_end && d_result, "null pointer");
  PL_REQUIRE(nbytes >= 0, "negative size");
  PL_REQUIRE(pl_dicom_encap_index_bytes(n_members, cap, tcap, head_bytes) >= 0,
             "1 <= n_members < 2^31, 1 <= cap, tcap <= 2^24, head_bytes a multiple of 16 up to PL_DICOM_ENCAP_MAX_HEAD");
  PL_REQUIRE(((uintptr_t)d_result & 15) == 0, "the result block must start on a 16-byte boundary");
  hipLaunchKernelGGL(enc_index_kernel, dim3((unsigned)n_members), dim3(PL_WAVE), 0, (hipStream_t)stream, d_bytes, nbytes, d_first,
                     d_end, n_members, cap, tcap, head_bytes, d_result);
  return pl_check_launch("pl_dicom_encap_index");
}

extern "C" int pl_copy_ranges(const unsigned char* d_src, int64_t src_bytes, unsigned char* d_dst, int64_t dst_bytes,
                              const int64_t* d_src_off, const int64_t* d_len, const int64_t* d_dst_off, int64_t n_ranges,
                              int64_t max_len, int32_t* d_status, void* stream) {
  PL_REQUIRE(d_src && d_dst && d_src_off && d_len && d_dst_off && d_status, "null pointer");
  PL_REQUIRE(n_ranges >= 1 && n_ranges <= 0x7fffffff, "1 <= n_ranges < 2^31");
  PL_REQUIRE(src_bytes >= 0 && dst_bytes >= 0 && max_len >= 0, "negative size");
  PL_REQUIRE(((uintptr_t)d_src & 3) == 0 && ((uintptr_t)d_dst & 3) == 0,
             "both buffers must start on a 4-byte boundary (ranges inside them may start anywhere)");
  int64_t bx = pl_cdiv(max_len / 16, (int64_t)kEncThreads * 4);
  if (bx < 1) bx = 1;
  if (bx > 2048) bx = 2048;
  const int64_t by = n_ranges < kEncMaxGridY ? n_ranges : kEncMaxGridY;
  hipLaunchKernelGGL(enc_copy_kernel, dim3((unsigned)bx, (unsigned)by), dim3(kEncThreads), 0, (hipStream_t)stream, d_src, src_bytes,
                     d_dst, dst_bytes, d_src_off, d_len, d_dst_off, n_ranges, d_status);
  return pl_check_launch("pl_copy_ranges");
}
