/* gmxmix_lstm_group.h -- the checkpoint of a whole LSTM group in one call: an extension of include/gmxmix.h, which it
 * includes.  libgmxmix.so exports both functions; they are declared here, not in gmxmix.h, whose list of entry
 * points is pinned by the project's ABI tests.  DESIGN.md section 4.19. */
#ifndef GMXMIX_LSTM_GROUP_H_
#define GMXMIX_LSTM_GROUP_H_

#include "gmxmix.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Checkpoint streams [first, first + count) of an LSTM group in one call.  Stream i's sections -- byte for byte what
 * gmx_lstm_export gives for it -- lie at long_buf + i * *long_stride and short_buf + i * *short_stride.  The strides
 * (5 560 200 and 1 458 256) are always filled when their pointers are not NULL.  Either buffer may be NULL: that half
 * is skipped; both NULL only sizes.  GMX_ERR_INVALID if a cap is below count * stride; nothing is written then.
 * The sections are laid out on the device (transposes and pitch changes included) and travel through pinned staging
 * buffers in slices of consecutive streams; no host copy of a bank is made. */
int gmx_lstm_group_export(gmx_lstm* l, int first, int count, void* long_buf, size_t long_cap,
                          void* short_buf, size_t short_cap, size_t* long_stride, size_t* short_stride);
/* The inverse; both halves are required.  long_bytes / short_bytes must be count * stride (GMX_ERR_FORMAT), and every
 * stream's header is validated as gmx_lstm_import validates it (epochs < 100, update_steps <= 3000, 0 <= bot_ <= mid_
 * <= top_ <= 255) BEFORE any bank is touched: a bad section anywhere leaves all banks as they were. */
int gmx_lstm_group_import(gmx_lstm* l, int first, int count, const void* long_buf, size_t long_bytes,
                          const void* short_buf, size_t short_bytes);

#ifdef __cplusplus
}
#endif
#endif /* GMXMIX_LSTM_GROUP_H_ */
