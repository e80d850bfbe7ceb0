// one database digit plan (HT = 1 high chunks) of the third scan shape: seed and consume kernels for every query plan
#include "tm_knn3_kernels.h"
namespace tmx {
TM_KNN3_DEFINE_HT(1)
}
